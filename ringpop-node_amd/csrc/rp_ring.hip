// rp_ring.hip — the consistent hash ring on MI355X.
//
// Replaces lib/ring/index.js (HashRing) + lib/ring/rbtree.js (RBTree). The red-black tree is
// an ordered map token -> owner with insert-if-absent and erase-by-key (rbtree.js:112-116,
// 152-232); here it is a sorted uint32 token array + owner array in HBM, rebuilt per
// addRemoveServers batch by: device farmhash of every replica string -> stable radix sort
// -> drop in-batch duplicates and tokens already present (first insert wins) -> parallel
// merge with the live array; removals mark-and-compact by token regardless of owner.
// A 2^B bucket index over the top token bits bounds each lookup's search.
//
// Hot path: batched lookup / lookupN (lib/ring/index.js:145-189). One thread per key;
// fixed-stride keys are staged through LDS with coalesced 16-B loads, hashed from
// registers (fh::hash32_words), searched bucket-first, walked for distinct owners, and the
// owner rows are staged back through LDS for coalesced stores.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ringpop_amd.h"
#include "rp_farmhash.h"
#include "rp_philox.h"
#include "rp_hashlong.h"
#include "rp_names.h"
#include "rp_prims.h"

namespace rp {

constexpr uint32_t NIL = 0xFFFFFFFFu;

static bool getenv_flag(const char* name) {
    const char* v = getenv(name);
    return v && *v && *v != '0';
}

struct RingView {
    const uint32_t* tok;
    const uint32_t* own;
    const uint32_t* bstart;  // 2^bbits + 1 entries
    uint32_t M;
    uint32_t shift;  // 32 - bbits

    // first index i in [0, M] with tok[i] >= h (RBTree upperBound semantics, rbtree.js:235-271)
    __device__ __forceinline__ uint32_t find(uint32_t h) const {
        const uint32_t b = h >> shift;
        uint32_t lo = bstart[b], hi = bstart[b + 1];
        while (lo < hi) {
            uint32_t mid = (lo + hi) >> 1;
            if (tok[mid] < h) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
    __device__ __forceinline__ uint32_t owner(uint32_t j) const { return own[j]; }
};

// Packed lookup layout: 2^B buckets on the top B token bits (B chosen for ~4 tokens per
// bucket); each entry is one uint32 = (token low 32-B bits) << B | owner, so owner ids must be
// < 2^B. A bucket plus its lookupN successors usually sits inside one 16-entry (64-B) window.
// The entry array is padded with 0xFFFFFFFF so window loads past M stay in bounds.
struct PackedView {
    const uint32_t* ent;
    const uint32_t* bstart;  // 2^B + 1 entries
    uint32_t M;
    uint32_t B;

    __device__ __forceinline__ uint32_t key_of(uint32_t h) const { return (h << B) >> 0; }
    __device__ __forceinline__ uint32_t find(uint32_t h) const {
        const uint32_t b = h >> (32 - B);
        const uint32_t key = h << B;  // the low 32-B bits of h, shifted over the owner field
        uint32_t lo = bstart[b], hi = bstart[b + 1];
        while (lo < hi) {
            uint32_t mid = (lo + hi) >> 1;
            if (ent[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
    __device__ __forceinline__ uint32_t owner(uint32_t j) const { return ent[j] & ((1u << B) - 1u); }
};

// Compact lookup layout (the C2 hot path). Sized so the whole table stays in one XCD's 4 MB L2
// (≈3.5 MB at 10k servers x 100 replicas; the packed layout's 8 MB missed ~half the time):
//   2^cb buckets on the top cb token bits, cb = floor(log2 M) (1-2 tokens per bucket);
//   idx[g] = {position of the first token of bucket 8g, 8 x 4-bit token counts of buckets
//   8g..8g+7} (8 B per 8 buckets); ent = 3 bytes per token, (fp << ob) | owner, where fp is
//   the top (24 - ob) bits of the token's low 32 - cb bits (all of them when they fit) and
//   owner < 2^ob. A key's bucket start is one 8-B load plus a nibble sum; its position and
//   successor owners come from one unaligned 16-B load of 5 entries. A key whose fingerprint
//   equals one in its bucket (only when fp drops bits) is deferred to the exact fix path.
struct CompactView {
    const uint8_t* ent;   // 3 B per token, M + kEnt3Pad entries (+16 B)
    const uint32_t* idx;  // 2 u32 per group of 8 buckets
    uint32_t M;
    uint32_t cb;   // bucket bits (>= 3)
    uint32_t ob;   // owner bits
    uint32_t fsh;  // fingerprint = (low 32 - cb bits of the hash) >> fsh
    uint32_t exact;  // fsh == 0: fingerprints are the whole residual
    uint32_t ablate;  // diagnostics only (RP_LOOKUP_ABLATE): 1 = no second windows, 2 = aligned windows
    uint32_t ent_bytes;  // allocated bytes of ent / idx (buffer-descriptor ranges of the lean kernel)
    uint32_t idx_bytes;
    uint32_t wpred;  // lean kernel: window 1 starts where the key's hash falls in its bucket (A/B:
                     // RP_LOOKUP_WPRED=0 starts it at the bucket start)
    // round 5: the hinted index (lookupN(3) in the lean kernel): per group of 8 buckets
    // {14-bit signed base - pred(g) | 8 x 2-bit window-start hints, nibble counts}, pred(g) =
    // g * M >> (cb - 3); hint h moves window 1's start by h - 1 entries (chosen at build time per
    // bucket so that the most of its hash range resolves in window 1). idxh null: no hints.
    const uint32_t* idxh;
};

// Exact view for the compact kernel's deferred keys: the bucket start comes from the compact
// index (one load) and the position from the exact wide tokens of that bucket, so a deferred
// key costs ~4 dependent loads instead of a full binary search.
struct CompactFixView {
    const uint32_t* tok;
    const uint32_t* own;
    const uint32_t* idx;
    RingView wide;  // buckets of 16+ tokens
    uint32_t M;
    uint32_t cb;

    __device__ __forceinline__ uint32_t find(uint32_t h) const {
        const uint32_t bsh = 32u - cb;
        const uint32_t g = h >> (bsh + 3u), s4 = ((h >> bsh) & 7u) * 4u;
        const uint32_t base = idx[2 * g], nib = idx[2 * g + 1];
        const uint32_t bc = (nib >> s4) & 15u;
        if (bc == 15u) return wide.find(h);
        const uint32_t below = nib & ((1u << s4) - 1u);
        const uint32_t x = (below & 0x0F0F0F0Fu) + ((below >> 4) & 0x0F0F0F0Fu);
        uint32_t i = base + ((x * 0x01010101u) >> 24);
        for (uint32_t j = 0; j < bc && tok[i] < h; j++) i++;
        return i;
    }
    __device__ __forceinline__ uint32_t owner(uint32_t j) const { return own[j]; }
};

// lookupN walk (lib/ring/index.js:157-189) with the result kept in registers (np <= MAXN).
// Visits positions i%M, i%M+1, ... cyclically, at most M of them, stopping once np
// distinct owners are collected. np <= 0 reproduces the reference's single loop body.
template <int MAXN, class View>
__device__ __forceinline__ int ring_walk(const View& rv, uint32_t i, int np, uint32_t (&res)[MAXN]) {
#pragma unroll
    for (int q = 0; q < MAXN; q++) res[q] = NIL;
    if (rv.M == 0) return 0;
    if (np <= 0) {
        if (i < rv.M) {
            res[0] = rv.owner(i);
            return 1;
        }
        return 0;
    }
    uint32_t j = (i == rv.M) ? 0u : i;
    if (MAXN == 1) {
        res[0] = rv.owner(j);
        return 1;
    }
    int cnt = 0;
    for (uint32_t steps = 0; steps < rv.M; steps++) {
        const uint32_t o = rv.owner(j);
        bool dup = false;
#pragma unroll
        for (int q = 0; q < MAXN; q++) dup |= (q < cnt) & (res[q] == o);
        if (!dup) {
#pragma unroll
            for (int q = 0; q < MAXN; q++) res[q] = (q == cnt) ? o : res[q];
            cnt++;
            if (cnt >= np) break;
        }
        j = (j + 1 == rv.M) ? 0u : j + 1;
    }
    return cnt;
}

// Unbounded walk writing straight to the output row (np > 8).
template <class View>
__device__ int ring_walk_global(const View& rv, uint32_t i, int np, uint32_t* row, uint32_t W) {
    for (uint32_t q = 0; q < W; q++) row[q] = NIL;
    if (rv.M == 0) return 0;
    if (np <= 0) {
        if (i < rv.M) {
            row[0] = rv.owner(i);
            return 1;
        }
        return 0;
    }
    uint32_t j = (i == rv.M) ? 0u : i;
    int cnt = 0;
    for (uint32_t steps = 0; steps < rv.M; steps++) {
        const uint32_t o = rv.owner(j);
        bool dup = false;
        for (int q = 0; q < cnt; q++)
            if (row[q] == o) {
                dup = true;
                break;
            }
        if (!dup) {
            row[cnt++] = o;
            if (cnt >= np) break;
        }
        j = (j + 1 == rv.M) ? 0u : j + 1;
    }
    return cnt;
}

namespace {

constexpr int kLkThreads = 256;
constexpr uint32_t kEntPad = 32;  // padding entries after M in the packed array
constexpr uint32_t kEnt3Pad = 16;  // padding entries after M in the compact array (+16 bytes)
constexpr int kDefaultKPL = 2;     // keys per lane in the probe kernel (RP_LOOKUP_KPL overrides)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Fixed-stride keys (LEN % 4 == 0, LEN > 24, e.g. 36-byte UUIDs): the hot kernel.
// Keys stream HBM -> registers -> LDS with 16-B non-temporal loads (read once; they must not
// evict the ring table from L2). The next tile's loads are issued before the current tile is
// hashed, so their HBM latency hides under the search. Each lane hashes its key from
// registers, searches, walks, and the owner rows leave through LDS as 16-B non-temporal stores.
// MODE is a diagnostic ablation (0 = full; 1 = write the hash; 2 = write the ring index).
template <int LEN, int MAXN, class View, int MODE = 0>
__global__ __launch_bounds__(kLkThreads) void k_lookupn_fixed(const uint8_t* __restrict__ keys, uint64_t n,
                                                              View rv, int np, uint32_t W,
                                                              uint32_t* __restrict__ out,
                                                              uint8_t* __restrict__ counts) {
    constexpr int W4 = LEN / 4;                       // dwords per key
    constexpr int V4 = kLkThreads * W4 / 4;           // 16-B vectors per tile
    constexpr int PER = (V4 + kLkThreads - 1) / kLkThreads;
    static_assert((kLkThreads * W4) % 4 == 0, "tile must be a whole number of 16-B vectors");
    __shared__ __attribute__((aligned(16))) uint32_t sk[kLkThreads * W4];
    __shared__ __attribute__((aligned(16))) uint32_t so[kLkThreads * MAXN];
    const int tid = threadIdx.x;
    const bool kvec = ((reinterpret_cast<uintptr_t>(keys) & 15) == 0);
    const bool ovec = ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
    const uint64_t ntiles = (n + kLkThreads - 1) / kLkThreads;
    const uint64_t nfull = n / kLkThreads;  // tiles with all 256 keys

    u32x4 pre[PER];
    auto issue = [&](uint64_t t) {
        const u32x4* s4 = reinterpret_cast<const u32x4*>(keys + t * kLkThreads * LEN);
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int k = tid + q * kLkThreads;
            if (k < V4) pre[q] = __builtin_nontemporal_load(s4 + k);
        }
    };
    uint64_t t = blockIdx.x;
    if (kvec && t < nfull) issue(t);
    for (; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * kLkThreads;
        const uint32_t cnt = (uint32_t)((n - base) < (uint64_t)kLkThreads ? (n - base) : kLkThreads);
        if (kvec && t < nfull) {
            u32x4* d4 = reinterpret_cast<u32x4*>(sk);
#pragma unroll
            for (int q = 0; q < PER; q++) {
                const int k = tid + q * kLkThreads;
                if (k < V4) d4[k] = pre[q];
            }
        } else {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(keys + base * LEN);
            for (uint32_t k = tid; k < cnt * W4; k += kLkThreads) sk[k] = src[k];
        }
        __syncthreads();
        const uint64_t tn = t + gridDim.x;
        if (kvec && tn < nfull) issue(tn);  // in flight while this tile is searched
        int c = 0;
        uint32_t res[MAXN];
        if ((uint32_t)tid < cnt) {
            uint32_t w[W4];
#pragma unroll
            for (int j = 0; j < W4; j++) w[j] = sk[tid * W4 + j];
            const uint32_t h = fh::hash32_words<LEN>(w);
            if constexpr (MODE == 1) {
#pragma unroll
                for (int q = 0; q < MAXN; q++) res[q] = h + q;
                c = 1;
            } else if constexpr (MODE == 2) {
                const uint32_t i = rv.find(h);
#pragma unroll
                for (int q = 0; q < MAXN; q++) res[q] = i + q;
                c = 1;
            } else {
                const uint32_t i = rv.find(h);
                c = ring_walk<MAXN>(rv, i, np, res);
            }
#pragma unroll
            for (int q = 0; q < MAXN; q++)
                if ((uint32_t)q < W) so[tid * W + q] = res[q];
            if (counts) counts[base + tid] = (uint8_t)c;
        }
        __syncthreads();
        uint32_t* dst = out + base * W;
        const uint32_t tot = cnt * W;
        if (ovec && cnt == kLkThreads && (tot & 3) == 0) {
            u32x4* d4 = reinterpret_cast<u32x4*>(dst);
            const u32x4* s4 = reinterpret_cast<const u32x4*>(so);
            for (uint32_t k = tid; k < tot / 4; k += kLkThreads) __builtin_nontemporal_store(s4[k], d4 + k);
        } else {
            for (uint32_t k = tid; k < tot; k += kLkThreads) dst[k] = so[k];
        }
        __syncthreads();
    }
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

// The C2 hot kernel (packed layout with ~1 token per bucket; lookup / lookupN with n <= 4;
// 36-byte keys). Every random access is ONE load instruction per key, so it costs one
// L1->L2 request (each lane of a wave instruction touching a different line is a separate
// request; PMC showed ~6 requests/key for a binary search + walk):
//   LDS key words -> farmhash32 -> [bucket lo, hi) as one 8-B load -> the 4 entries at lo as
//   one 16-B load -> position i = lo + #(entries < key) and the successor owners, from
//   registers; only when the successors run past those 4 entries, one more 16-B load at i.
// Each lane owns KPL keys of a 256*KPL-key tile, so each dependent trip serves KPL keys.
// Keys the 4-entry window cannot answer exactly (bucket longer than 4 with every entry below
// the key, positions within 3 of the end of the ring, repeated owners among the successors)
// are appended to a slow list and finished by k_lookupn_fix (binary search + the exact walk).
template <int LEN, int KPL, int MODE = 0>
__global__ __launch_bounds__(kLkThreads) void k_lookupn_probe(const uint8_t* __restrict__ keys, uint64_t n,
                                                              PackedView rv, int np, uint32_t W,
                                                              uint32_t* __restrict__ out,
                                                              uint8_t* __restrict__ counts,
                                                              uint32_t* __restrict__ slow_list,
                                                              uint32_t* __restrict__ nslow) {
    constexpr int W4 = LEN / 4;
    constexpr int TK = kLkThreads * KPL;
    constexpr int V4 = TK * W4 / 4;
    constexpr int PER = (V4 + kLkThreads - 1) / kLkThreads;
    static_assert((TK * W4) % 4 == 0, "tile must be whole 16-B vectors");
    // one LDS buffer: key words until every lane has hashed, then the owner rows
    constexpr int SK = TK * W4, SO = TK * 4;
    __shared__ __attribute__((aligned(16))) uint32_t lds[SK > SO ? SK : SO];
    uint32_t* const sk = lds;
    uint32_t* const so = lds;
    const int tid = threadIdx.x;
    const bool kvec = ((reinterpret_cast<uintptr_t>(keys) & 15) == 0);
    const bool ovec = ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
    const uint64_t ntiles = (n + TK - 1) / TK;
    const uint32_t B = rv.B;
    const uint32_t omask = (1u << B) - 1u;
    const int need = np <= 0 ? 1 : np;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * TK;
        const uint32_t cnt = (uint32_t)((n - base) < (uint64_t)TK ? (n - base) : TK);
        if (kvec && cnt == TK) {
            const u32x4* s4 = reinterpret_cast<const u32x4*>(keys + base * LEN);
            u32x4 pre[PER];
#pragma unroll
            for (int q = 0; q < PER; q++) {
                const int k = tid + q * kLkThreads;
                if (k < V4) pre[q] = __builtin_nontemporal_load(s4 + k);
            }
            u32x4* d4 = reinterpret_cast<u32x4*>(sk);
#pragma unroll
            for (int q = 0; q < PER; q++) {
                const int k = tid + q * kLkThreads;
                if (k < V4) d4[k] = pre[q];
            }
        } else {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(keys + base * LEN);
            for (uint32_t k = tid; k < cnt * W4; k += kLkThreads) sk[k] = src[k];
        }
        __syncthreads();
        uint32_t h[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const uint32_t kk = tid + k * kLkThreads;
            uint32_t w[W4];
#pragma unroll
            for (int j = 0; j < W4; j++) w[j] = sk[(kk < cnt ? kk : 0) * W4 + j];
            h[k] = fh::hash32_words<LEN>(w);
        }
        __syncthreads();  // sk is reused as so below
        if constexpr (MODE == 1) {
#pragma unroll
            for (int k = 0; k < KPL; k++) {
                const uint32_t kk = tid + k * kLkThreads;
                if (kk < cnt) {
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if ((uint32_t)q < W) so[kk * W + q] = h[k] + q;
                }
            }
        } else {
            u32x2 bb[KPL];
#pragma unroll
            for (int k = 0; k < KPL; k++)
                bb[k] = *reinterpret_cast<const u32x2_a4*>(rv.bstart + (h[k] >> (32 - B)));
            u32x4 win[KPL];
#pragma unroll
            for (int k = 0; k < KPL; k++) win[k] = *reinterpret_cast<const u32x4_a4*>(rv.ent + bb[k].x);
#pragma unroll
            for (int k = 0; k < KPL; k++) {
                const uint32_t kk = tid + k * kLkThreads;
                const uint32_t lo = bb[k].x, hi = bb[k].y;
                const uint32_t key = h[k] << B;
                const uint32_t len = hi - lo;
                const uint32_t c = (0u < len && win[k].x < key) + (1u < len && win[k].y < key) +
                                   (2u < len && win[k].z < key) + (3u < len && win[k].w < key);
                const uint32_t i = lo + c;
                bool slow = (c == 4u && len > 4u) | (i + 3u >= rv.M);
                uint32_t e0, e1, e2, e3;
                if (4u - c >= (uint32_t)need) {
                    // successors i.. are win[c..3]
                    const uint32_t a0 = (c & 1) ? win[k].y : win[k].x, a1 = (c & 1) ? win[k].z : win[k].y;
                    const uint32_t a2 = (c & 1) ? win[k].w : win[k].z, a3 = win[k].w;
                    e0 = (c & 2) ? a2 : a0;
                    e1 = (c & 2) ? a3 : a1;
                    e2 = a2;
                    e3 = a3;
                } else {
                    const u32x4 sc = *reinterpret_cast<const u32x4_a4*>(rv.ent + (i < rv.M ? i : 0u));
                    e0 = sc.x;
                    e1 = sc.y;
                    e2 = sc.z;
                    e3 = sc.w;
                }
                uint32_t res[4] = {NIL, NIL, NIL, NIL};
                uint32_t rc = 1;
                if constexpr (MODE == 2) {
                    res[0] = i;
                    res[1] = i + 1;
                    res[2] = i + 2;
                    res[3] = i + 3;
                } else {
                    const uint32_t o0 = e0 & omask, o1 = e1 & omask, o2 = e2 & omask, o3 = e3 & omask;
                    // distinct owners in visit order (lib/ring/index.js:173-186)
                    res[0] = o0;
                    const uint32_t oq[3] = {o1, o2, o3};
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        const uint32_t o = oq[q];
                        const bool dup = (o == res[0]) | (rc > 1 && o == res[1]) | (rc > 2 && o == res[2]);
                        if (!dup && (int)rc < need) {
                            res[1] = rc == 1 ? o : res[1];
                            res[2] = rc == 2 ? o : res[2];
                            res[3] = rc == 3 ? o : res[3];
                            rc++;
                        }
                    }
                    slow |= (int)rc < need;  // repeated owners: the walk must go further
                }
                if (kk < cnt) {
                    if (slow) {
                        const uint32_t pos = atomicAdd(nslow, 1u);
                        slow_list[pos] = (uint32_t)(base + kk);
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if ((uint32_t)q < W) so[kk * W + q] = res[q];
                    if (counts) counts[base + kk] = (uint8_t)rc;
                }
            }
        }
        __syncthreads();
        uint32_t* dst = out + base * W;
        const uint32_t tot = cnt * W;
        if (ovec && cnt == TK && (tot & 3) == 0) {
            u32x4* d4 = reinterpret_cast<u32x4*>(dst);
            const u32x4* s4 = reinterpret_cast<const u32x4*>(so);
            for (uint32_t k = tid; k < tot / 4; k += kLkThreads) __builtin_nontemporal_store(s4[k], d4 + k);
        } else {
            for (uint32_t k = tid; k < tot; k += kLkThreads) dst[k] = so[k];
        }
        __syncthreads();
    }
}

typedef uint32_t u32x4_a1 __attribute__((ext_vector_type(4), aligned(1)));

// the 5 whole 3-byte entries in a 16-byte window
__device__ __forceinline__ void ent5(const u32x4_a1 v, uint32_t (&e)[5]) {
    e[0] = v.x & 0xFFFFFFu;
    e[1] = (v.x >> 24) | ((v.y & 0xFFFFu) << 8);
    e[2] = (v.y >> 16) | ((v.z & 0xFFu) << 16);
    e[3] = v.z >> 8;
    e[4] = v.w & 0xFFFFFFu;
}

// distinct owners in visit order (lib/ring/index.js:173-186) from window entries j >= off
__device__ __forceinline__ uint32_t dedupe5(const uint32_t (&e)[5], uint32_t off, uint32_t omask, uint32_t need,
                                            uint32_t (&res)[4]) {
    uint32_t rc = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint32_t o = e[j] & omask;
        const bool dup = (rc > 0 && o == res[0]) | (rc > 1 && o == res[1]) | (rc > 2 && o == res[2]);
        if ((uint32_t)j >= off && !dup && rc < need) {
            res[0] = rc == 0 ? o : res[0];
            res[1] = rc == 1 ? o : res[1];
            res[2] = rc == 2 ? o : res[2];
            res[3] = rc == 3 ? o : res[3];
            rc++;
        }
    }
    return rc;
}

constexpr uint32_t kSlowPerTile = 32;  // deferred-key slots per tile of the compact kernel

// The C2 hot kernel over the compact layout: KPL keys per lane, all of a lane's random loads
// issued together (the index records, then the entry windows, then any second windows), so
// each dependent trip overlaps KPL keys. Whole tiles only (the launcher sends the tail to the
// generic kernel), 16-B aligned keys and output rows of NEED owners. Keys stream HBM -> LDS
// with 16-B non-temporal loads; owner rows leave through LDS as 16-B non-temporal stores.
// Per key: window 1 = the 5 entries at the bucket start. If the bucket has more than 5 tokens
// and all 5 are below the key, window 2 continues the search at lo + 5; if the owners run
// past window 1, window 2 starts at the position. Deferred to the exact fix path (per-tile
// slot lists, no global atomics): a fingerprint tie, a bucket of more than 10 tokens, a
// position within 10 of the ring end (wrap), more repeated owners than the windows cover.
template <int KPL, int NEED>
__global__ __launch_bounds__(kLkThreads) void k_lookupn_compact(const uint8_t* __restrict__ keys, uint64_t ntiles,
                                                                CompactView cv, uint32_t* __restrict__ out,
                                                                uint8_t* __restrict__ counts,
                                                                uint32_t* __restrict__ slow_list,
                                                                uint32_t* __restrict__ slow_cnt) {
    constexpr int LEN = 36, W4 = LEN / 4;
    constexpr int TK = kLkThreads * KPL;
    constexpr int V4 = TK * W4 / 4;
    constexpr int PER = (V4 + kLkThreads - 1) / kLkThreads;
    static_assert((TK * W4) % 4 == 0 && (TK * NEED) % 4 == 0, "tile must be whole 16-B vectors");
    constexpr int SK = TK * W4, SO = TK * NEED;
    __shared__ __attribute__((aligned(16))) uint32_t lds[SK > SO ? SK : SO];
    __shared__ uint32_t nslow_tile;
    uint32_t* const sk = lds;
    uint32_t* const so = lds;
    const int tid = threadIdx.x;
    const uint32_t omask = (1u << cv.ob) - 1u;
    const uint32_t bsh = 32u - cv.cb;
    const uint32_t rmask = (1u << bsh) - 1u;
    const u32x2* idx2 = reinterpret_cast<const u32x2*>(cv.idx);
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * TK;
        {
            const u32x4* s4 = reinterpret_cast<const u32x4*>(keys + base * LEN);
            u32x4 pre[PER];
#pragma unroll
            for (int q = 0; q < PER; q++) {
                const int k = tid + q * kLkThreads;
                if (k < V4) pre[q] = __builtin_nontemporal_load(s4 + k);
            }
#pragma unroll
            for (int q = 0; q < PER; q++) {
                const int k = tid + q * kLkThreads;
                if (k < V4) reinterpret_cast<u32x4*>(sk)[k] = pre[q];
            }
        }
        if (tid == 0) nslow_tile = 0;
        __syncthreads();
        uint32_t h[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            uint32_t w[W4];
#pragma unroll
            for (int j = 0; j < W4; j++) w[j] = sk[(tid + k * kLkThreads) * W4 + j];
            h[k] = fh::hash32_words<LEN>(w);
        }
        __syncthreads();  // sk is reused as so below
        u32x2 rec[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) rec[k] = idx2[h[k] >> (bsh + 3u)];
        uint32_t lo[KPL], bc[KPL];
        u32x4_a1 win[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const uint32_t s4 = ((h[k] >> bsh) & 7u) * 4u;
            const uint32_t below = rec[k].y & ((1u << s4) - 1u);
            const uint32_t x = (below & 0x0F0F0F0Fu) + ((below >> 4) & 0x0F0F0F0Fu);
            lo[k] = rec[k].x + ((x * 0x01010101u) >> 24);
            bc[k] = (rec[k].y >> s4) & 15u;
            win[k] = *reinterpret_cast<const u32x4_a1*>(cv.ent + ((3ull * lo[k]) & (cv.ablate == 2 ? ~15ull : ~0ull)));
        }
        uint32_t res[KPL][4], rc[KPL], ipos[KPL], kfp[KPL];
        bool slow[KPL], search[KPL], again[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            uint32_t e[5];
            ent5(win[k], e);
            kfp[k] = (h[k] & rmask) >> cv.fsh;
            uint32_t lt = 0;
            bool tie = false;
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const uint32_t f = e[j] >> cv.ob;
                const bool inb = (uint32_t)j < bc[k];
                lt += (inb && f < kfp[k]);
                tie |= (inb && f == kfp[k]);
            }
            search[k] = lt == 5u && bc[k] > 5u;  // the position lies past window 1
            ipos[k] = lo[k] + lt;
            slow[k] = (tie && !cv.exact) | (lo[k] + 10u > cv.M);
            res[k][0] = res[k][1] = res[k][2] = res[k][3] = NIL;
            rc[k] = search[k] ? 0u : dedupe5(e, lt, omask, NEED, res[k]);
            again[k] = !slow[k] && (search[k] || rc[k] < (uint32_t)NEED) && cv.ablate != 1;
        }
#pragma unroll
        for (int k = 0; k < KPL; k++)
            if (again[k]) win[k] = *reinterpret_cast<const u32x4_a1*>(cv.ent + 3ull * ipos[k]);
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            if (again[k]) {
                uint32_t e[5];
                ent5(win[k], e);
                uint32_t off = 0;
                if (search[k]) {  // window 2 holds bucket entries 5..9
                    bool tie = false;
#pragma unroll
                    for (int j = 0; j < 5; j++) {
                        const uint32_t f = e[j] >> cv.ob;
                        const bool inb = (uint32_t)j + 5u < bc[k];
                        off += (inb && f < kfp[k]);
                        tie |= (inb && f == kfp[k]);
                    }
                    slow[k] |= (tie && !cv.exact) | (off == 5u && bc[k] > 10u);
                }
                res[k][0] = res[k][1] = res[k][2] = res[k][3] = NIL;
                rc[k] = dedupe5(e, off, omask, NEED, res[k]);
                slow[k] |= rc[k] < (uint32_t)NEED;
            }
            const uint32_t kk = tid + k * kLkThreads;
            if (slow[k]) {
                const uint32_t pos = atomicAdd(&nslow_tile, 1u);
                if (pos < kSlowPerTile) slow_list[t * kSlowPerTile + pos] = (uint32_t)kk;
            }
#pragma unroll
            for (int q = 0; q < NEED; q++) so[kk * NEED + q] = res[k][q];
            if (counts) counts[base + kk] = (uint8_t)rc[k];
        }
        __syncthreads();
        if (tid == 0) slow_cnt[t] = nslow_tile;
        u32x4* d4 = reinterpret_cast<u32x4*>(out + base * NEED);
        const u32x4* s4 = reinterpret_cast<const u32x4*>(so);
#pragma unroll
        for (int k = tid; k < TK * NEED / 4; k += kLkThreads) __builtin_nontemporal_store(s4[k], d4 + k);
        __syncthreads();
    }
}

// The exact position and walk of a deferred key on the compact layout with the dependent trips
// cut: the bucket's tokens are compared four at a time (one vector load for a bucket of <= 4) and
// the next 8 owners come in two vector loads; the result equals ring_walk's (the general walk
// takes over when 8 entries do not hold np distinct owners or the ring end is near).
__device__ __forceinline__ int compact_fix_walk(const CompactFixView& fv, uint32_t h, int np, uint32_t (&res)[4]) {
    if (np < 1 || np > 4) return ring_walk<4>(fv, fv.find(h), np, res);
    const uint32_t bsh = 32u - fv.cb;
    const uint32_t g = h >> (bsh + 3u), s4 = ((h >> bsh) & 7u) * 4u;
    const u32x2 rec = *reinterpret_cast<const u32x2*>(fv.idx + 2ull * g);
    const uint32_t bc = (rec.y >> s4) & 15u;
    uint32_t i;
    if (bc == 15u) {
        i = fv.wide.find(h);
    } else {
        const uint32_t below = rec.y & ((1u << s4) - 1u);
        const uint32_t x = (below & 0x0F0F0F0Fu) + ((below >> 4) & 0x0F0F0F0Fu);
        i = rec.x + ((x * 0x01010101u) >> 24);
        uint32_t lt = 0;
        for (uint32_t j = 0; j < bc; j += 4) {
            if (i + j + 4 <= fv.M) {
                const u32x4_a1 v = *reinterpret_cast<const u32x4_a1*>(fv.tok + i + j);
                lt += (j < bc && v.x < h) + (j + 1 < bc && v.y < h) + (j + 2 < bc && v.z < h) + (j + 3 < bc && v.w < h);
            } else {
                for (uint32_t q = j; q < bc && q < j + 4; q++) lt += fv.tok[i + q] < h;
            }
        }
        i += lt;  // tokens are sorted: the count below h is the position
    }
    const uint32_t p = (i == fv.M) ? 0u : i;
    if (p + 8 <= fv.M) {
        const u32x4_a1 a = *reinterpret_cast<const u32x4_a1*>(fv.own + p);
        const u32x4_a1 b = *reinterpret_cast<const u32x4_a1*>(fv.own + p + 4);
        const uint32_t o[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int q = 0; q < 4; q++) res[q] = NIL;
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            bool dup = false;
#pragma unroll
            for (int q = 0; q < 4; q++) dup |= (q < cnt) & (res[q] == o[j]);
            if (!dup && cnt < np) {
#pragma unroll
                for (int q = 0; q < 4; q++) res[q] = (q == cnt) ? o[j] : res[q];
                cnt++;
            }
        }
        if (cnt >= np) return cnt;
    }
    return ring_walk<4>(fv, i, np, res);
}

template <class View>
__device__ __forceinline__ int fix_walk(const View& rv, uint32_t h, int np, uint32_t (&res)[4]) {
    if constexpr (std::is_same<View, CompactFixView>::value)
        return compact_fix_walk(rv, h, np, res);
    else
        return ring_walk<4>(rv, rv.find(h), np, res);
}

// One deferred key redone exactly: hash, exact position, the reference walk; its row and count
// overwrite what the compact kernel stored.
template <class View>
__device__ __forceinline__ void lookupn_redo(const uint8_t* __restrict__ keys, const View& rv, int np, uint32_t W,
                                             uint32_t* __restrict__ out, uint8_t* __restrict__ counts, uint64_t k) {
    uint32_t w[9];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(keys + k * 36);
#pragma unroll
    for (int j = 0; j < 9; j++) w[j] = src[j];
    const uint32_t h = fh::hash32_words<36>(w);
    uint32_t res[4];
    const int cnt = fix_walk(rv, h, np, res);
    uint32_t* row = out + k * W;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if ((uint32_t)q < W) row[q] = res[q];
    if (counts) counts[k] = (uint8_t)cnt;
}

// Phase cycle counters of the lean kernel (diagnostics only: built with -DRP_LK_PROF by
// tools/build_prof.sh; the product build has none of this). A wave stamps s_memtime at each
// phase boundary, the stamp depending on the phase's last result; the per-phase sums over all
// waves land in g_lk_prof (printed by lookupn_compact under RP_LK_PROF_PRINT).
#ifdef RP_LK_PROF
__device__ unsigned long long g_lk_prof[10];
#define LK_T(var, dep) \
    uint64_t var;      \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var) : "v"(dep))
#else
#define LK_T(var, dep)
#endif

// The C2 hot kernel, lean form (round 2): the same layout, loads and results as
// k_lookupn_compact, with fewer vector instructions per key (the SQ counters put that kernel at
// ~2.9x the VALU issue of the hash-only ablation).
//   - The index record and the window come through buffer descriptors with 32-bit offsets (no
//     64-bit address arithmetic); the nibble sum is two v_sad_u8.
//   - Window 1 resolves a key in one straight-line pass when its position is at most 5 - NEED
//     entries into the window and the NEED owners there are distinct: the fingerprint tests
//     compare whole entries against kfp << ob, the owners are picked by the position.
//   - The ~8 % of keys that need a second window (the position lies further, a long bucket, or
//     a repeated owner) are appended to a per-wave list (ballot + mbcnt, 64 slots in LDS); the
//     wave then finishes them one key per lane, so the second-window code runs once per wave
//     instead of once per key slot. Keys past the list go to the exact fix path, like ties and
//     positions near the ring end.
// HS: the tile's keys pass through LDS in HS slices (all loads issued first, held in registers),
// so the key stage takes 1/HS of the LDS and more workgroups fit a CU (A/B).
// (Forcing 5 waves per SIMD with __launch_bounds__ spills 8 VGPRs and ran 1.05 against 0.91 ms,
// profiles/r03/ab_lookup_occ.json: the 119-121 VGPRs and 4 waves per SIMD stay.)
// FUSE: the workgroup finishes its own tiles' deferred keys after its last tile (one thread per
// list slot, 8 tiles at a time) instead of k_lookupn_fix_tiles (A/B: RP_LOOKUP_FUSEFIX).
// STG: how the key tile reaches LDS. 0: every lane loads all its 16-B pieces of the tile into
// registers first (PER x u32x4 held), then the slices go through LDS one after another. 1: the
// slices are DMA'd global -> LDS (global_load_lds_dwordx4, no VGPR destination) into a ring of
// two slice buffers, slice s + 2 issued as soon as slice s is hashed (A/B: RP_LOOKUP_STG=1).
// The lean kernel's timing ablations (RP_LOOKUP_ABLATE, round 5) exist only in a diagnostics
// build (-DRP_LK_ABLATE, tools/build_prof.sh). Read at run time (as from r05a to r05au), their
// uniform branches around the index and window loads split the loads' clusters: 3,394
// instructions and 181 branches against 3,191 and 139, 0.926 against 0.886 ms per 2^26-key step
// on one box, below round 4's kernel (0.903; profiles/r05/r05aw/).
#ifdef RP_LK_ABLATE
#define RP_LKA(cv) ((cv).ablate)
#else
#define RP_LKA(cv) 0u
#endif
constexpr uint32_t kLkAG = 64;  // second-window list slots per wave (8 % of 64 * KPL keys: ~41 at KPL 8)

// The lean lookup's per-key stages, shared by k_lookupn_lean and k_lookupn_sorted: the index
// record, window 1's start and load, the straight-line resolve with the per-wave second-window
// list, and the listed keys' finish. KB: bits of a key's tile slot in a list word (2^KB >= the
// tile's keys). A deferred key's tile slot goes to the caller's `defer`.
template <int NEED, int KB>
struct LkStages {
    static constexpr uint32_t SPAN = 5 - NEED;  // last window-1 position that still holds NEED entries
    const CompactView& cv;
    const uint32_t omask, obit, bsh, rmask;
    const __amdgpu_buffer_rsrc_t ent_r;
    // lookupN(3) reads the hinted index when the ring has one (round 5; RP_LOOKUP_HINT=0: A/B)
    const bool hinted;
    const __amdgpu_buffer_rsrc_t idx_r;

    __device__ __forceinline__ explicit LkStages(const CompactView& v)
        : cv(v), omask((1u << v.ob) - 1u), obit(1u << v.ob), bsh(32u - v.cb), rmask((1u << (32u - v.cb)) - 1u),
          ent_r(__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(v.ent), 0, (int)v.ent_bytes, 0x00020000)),
          hinted(NEED == 3 && v.idxh != nullptr && !(RP_LKA(v) & 4u)),
          idx_r(__builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(hinted ? v.idxh : v.idx), 0,
                                                  (int)v.idx_bytes, 0x00020000)) {}

    __device__ __forceinline__ u32x4 load16(uint32_t pos) const {
        return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ent_r, (int)(3u * pos), 0, 0));
    }
    static __device__ __forceinline__ void ent5v(const u32x4 v, uint32_t (&e)[5]) {
        e[0] = v.x & 0xFFFFFFu;
        e[1] = (v.x >> 24) | ((v.y & 0xFFFFu) << 8);
        e[2] = (v.y >> 16) | ((v.z & 0xFFu) << 16);
        e[3] = v.z >> 8;
        e[4] = v.w & 0xFFFFFFu;
    }
    // Window 1's first entry within the bucket (round 3): the key's position in a bucket of bc
    // tokens is about bc times its place in the bucket's hash range (r), so the window starts at
    // max(0, floor(r bc) - 1). A window at w > 0 resolves positions w+1..w+2 (entry w below the key
    // is the guard), one at 0 positions 0..2: 3.6 % of keys need a second window instead of 9.9 %
    // (Poisson buckets of 1.9 tokens; lookupN(2): 3.3 % -> 1.6 %). Long buckets (> 10) keep w = 0,
    // and so does lookup (NEED 1), whose window at 0 already resolves positions 0..4 (0.9 % of keys
    // past it against 1.5 % with the predicted start).
    // hint (the hinted index): the start moves by hint - 1 entries (1 = the plain prediction)
    __device__ __forceinline__ uint32_t wstart(uint32_t hk, uint32_t bck, uint32_t hint) const {
        const int fl = (int)((((hk << cv.cb) >> 24) * bck) >> 8) - 2 + (int)hint;
        return (NEED >= 2 && cv.wpred && bck <= 10u && fl > 0) ? (uint32_t)fl : 0u;
    }
    // the index trip: the 8-B record of the key's group of 8 buckets
    __device__ __forceinline__ u32x2 index_rec(uint32_t hk) const {
        if (RP_LKA(cv) & 4u)  // diagnostics: no index trip (a record made from the hash)
            return u32x2{(uint32_t)(((uint64_t)hk * (cv.M - 32u)) >> 32), hk & 0x11111111u};
        return __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(idx_r, (int)((hk >> (bsh + 3u)) * 8u), 0, 0));
    }
    // the window trip: the bucket start lo, its token count bc, window 1's start ws; returns the window
    __device__ __forceinline__ u32x4 window(uint32_t hk, const u32x2 rec, uint32_t& lo, uint32_t& bc, uint32_t& ws) const {
        const uint32_t s4 = ((hk >> bsh) & 7u) * 4u;
        const uint32_t below = rec.y & ((1u << s4) - 1u);
        uint32_t base = rec.x, hint = 1u;
        if (hinted) {  // base = pred(g) + the 14-bit delta; the bucket's 2-bit hint
            const uint32_t g = hk >> (bsh + 3u);
            base = (uint32_t)(((uint64_t)g * cv.M) >> (cv.cb - 3u)) + (uint32_t)((int32_t)(rec.x << 18) >> 18);
            hint = (rec.x >> (14u + (s4 >> 1))) & 3u;
        }
        lo = base + __builtin_amdgcn_sad_u8(below & 0x0F0F0F0Fu, 0u,
                                            __builtin_amdgcn_sad_u8((below >> 4) & 0x0F0F0F0Fu, 0u, 0u));
        bc = (rec.y >> s4) & 15u;
        ws = wstart(hk, bc, hint);
        if (RP_LKA(cv) & 26u) {  // diagnostics: 2 = windows rounded down to 16 B (no line crossing);
                                // 8 = no window trip (entries made from the record); 16 = windows
                                // rounded down to 4 B (dword-aligned, still crossing lines)
            const uint32_t pos = lo + ws;
            return (RP_LKA(cv) & 8u) ? u32x4{rec.x, rec.y, hk, pos}
                                     : __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                    ent_r, (int)((3u * pos) & ((RP_LKA(cv) & 2u) ? ~15u : ~3u)), 0, 0));
        }
        return load16(lo + ws);
    }
    // Window 1 of the key at tile slot kk: its row goes to so (and its count to cnt, the tile's
    // counts or null) when the window resolves it; else it joins the wave's list agw (nag: the
    // wave-uniform list length), or is deferred. Every lane of the wave calls this together.
    template <class Defer>
    __device__ __forceinline__ void resolve(const u32x4 win, uint32_t hk, uint32_t lo, uint32_t bc, uint32_t w,
                                            uint32_t kk, uint32_t& nag, uint32_t (*agw)[kLkAG], uint32_t* so,
                                            uint8_t* cnt, Defer&& defer) const {
        uint32_t e[5];
        ent5v(win, e);
        const uint32_t K = ((hk & rmask) >> cv.fsh) << cv.ob;
        uint32_t lt = 0;  // in-bucket window entries below the key: the position is lo + w + lt
        bool tie = false;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const bool inb = (uint32_t)j + w < bc;
            lt += (inb && e[j] < K);
            tie |= (inb && e[j] - K < obit);
        }
        uint32_t r[NEED];
#pragma unroll
        for (int q = 0; q < NEED; q++) {
            uint32_t v = e[q] & omask;
#pragma unroll
            for (uint32_t d = 1; d <= SPAN; d++) v = lt == d ? (e[q + d] & omask) : v;
            r[q] = v;
        }
        bool dup = false;
#pragma unroll
        for (int a = 0; a < NEED; a++)
#pragma unroll
            for (int b = a + 1; b < NEED; b++) dup |= r[a] == r[b];
        bool slow = (tie && !cv.exact) | (lo + 20u > cv.M);
        const bool under = w > 0u && lt == 0u;  // the key lies before window 1's first entry
        const bool again = !slow && (lt > SPAN || dup || under) && !(RP_LKA(cv) & 1u);  // 1: diagnostics
        const uint64_t m = __ballot(again);
        const uint32_t pos = nag + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        nag += (uint32_t)__popcll(m);
        if (again) {
            if (pos < kLkAG) {
                // under: search from w - 2 (the position is at most w), guarded when > 0; past
                // window 1 inside the bucket: search on from w + 5; else the position is known
                const uint32_t b0 = under ? (w > 2u ? w - 2u : 0u) : w + 5u;
                const bool search = under || (lt == 5u && bc > w + 5u);
                agw[0][pos] = lo + (search ? b0 : w + lt);
                agw[1][pos] = K;
                agw[2][pos] = kk | (bc << KB) | ((uint32_t)search << (KB + 4)) | ((search ? b0 : 0u) << (KB + 5)) |
                              ((uint32_t)(under && b0 > 0u) << (KB + 9));
            } else {
                slow = true;
            }
        } else {
#pragma unroll
            for (int q = 0; q < NEED; q++) so[kk * NEED + q] = r[q];
            if (cnt) cnt[kk] = (uint8_t)NEED;
        }
        if (slow) defer(kk);
    }
    // a listed key's second window (held by one lane): finish it, write its row into `row`
    template <class Defer>
    __device__ __forceinline__ void finish2(const u32x4 win, uint32_t K, uint32_t w2, uint32_t* row, uint8_t* cnt,
                                            Defer&& defer) const {
        const uint32_t kk = w2 & ((1u << KB) - 1u), bck = (w2 >> KB) & 15u, b0 = (w2 >> (KB + 5)) & 15u;
        uint32_t e2[5];
        ent5v(win, e2);
        uint32_t off = 0;
        bool slow = false;
        if ((w2 >> (KB + 4)) & 1u) {  // window 2 holds bucket entries b0..b0+4: search it
            bool tie = false;
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const bool inb = (uint32_t)j + b0 < bck;
                off += (inb && e2[j] < K);
                tie |= (inb && e2[j] - K < obit);
            }
            // past this window too; or (guard) the key may lie before entry b0
            slow = (tie && !cv.exact) | (off == 5u && bck > b0 + 5u) | (((w2 >> (KB + 9)) & 1u) && off == 0u);
        }
        uint32_t res[4] = {NIL, NIL, NIL, NIL};
        const uint32_t rc = dedupe5(e2, off, omask, NEED, res);
        slow |= rc < (uint32_t)NEED;
        if (slow) defer(kk);
#pragma unroll
        for (int q = 0; q < NEED; q++) row[kk * NEED + q] = res[q];
        if (cnt) cnt[kk] = (uint8_t)rc;
    }
};

// The key stage (STG 0): every lane loads all its 16-B pieces of the tile of THREADS * KPL keys
// into registers first (non-temporal), then the HS slices pass through the LDS stage sk one after
// another and are hashed: h[k] is the hash of the key at tile slot tid + k * THREADS. `issued`
// runs once the loads are issued, `arrived` once the first slice is in LDS.
// WAVE: THREADS is 64 and the tile is one wave's own (sk: the wave's own LDS stage, tid: the
// lane): the slices are exchanged between the wave's lanes only, with no workgroup barrier.
template <int THREADS, int KPL, int HS, bool WAVE = false, class Issued, class Arrived>
__device__ __forceinline__ void lk_key_stage(const uint8_t* __restrict__ tile_keys, uint32_t* sk, int tid,
                                             uint32_t (&h)[KPL], Issued&& issued, Arrived&& arrived) {
    constexpr int LEN = 36, W4 = LEN / 4;
    constexpr int V4 = THREADS * KPL * W4 / 4;
    constexpr int PER = (V4 + THREADS - 1) / THREADS;
    constexpr int VS = V4 / HS;  // 16-B vectors per slice
    static_assert(KPL % HS == 0 && V4 % HS == 0, "slices of whole keys");
    const u32x4* s4 = reinterpret_cast<const u32x4*>(tile_keys);
    u32x4 pre[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int k = tid + q * THREADS;
        if (k < V4) pre[q] = __builtin_nontemporal_load(s4 + k);
    }
    static_assert(!WAVE || THREADS == 64, "a wave's own tile");
    auto meet = [] {
        if constexpr (WAVE) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else {
            __syncthreads();
        }
    };
    issued();
#pragma unroll
    for (int hs = 0; hs < HS; hs++) {
        if (hs) meet();  // the previous slice is hashed
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int k = tid + q * THREADS;
            if (k >= hs * VS && k < (hs + 1) * VS) reinterpret_cast<u32x4*>(sk)[k - hs * VS] = pre[q];
        }
        meet();
        if (hs == 0) arrived();
#pragma unroll
        for (int k = hs * (KPL / HS); k < (hs + 1) * (KPL / HS); k++) {
            uint32_t w[W4];
#pragma unroll
            for (int j = 0; j < W4; j++) w[j] = sk[(tid + (k - hs * (KPL / HS)) * THREADS) * W4 + j];
            h[k] = fh::hash32_words<LEN>(w);
        }
    }
}

template <int KPL, int NEED, int HS = 1, bool FUSE = false, int STG = 0, int LH = 1>
__global__ __launch_bounds__(kLkThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_lookupn_lean(const uint8_t* __restrict__ keys, uint64_t ntiles,
                                                             CompactView cv, uint32_t* __restrict__ out,
                                                             uint8_t* __restrict__ counts,
                                                             uint32_t* __restrict__ slow_list,
                                                             uint32_t* __restrict__ slow_cnt, CompactFixView fv,
                                                             int np) {
    constexpr int LEN = 36, W4 = LEN / 4;
    constexpr int TK = kLkThreads * KPL;
    constexpr int V4 = TK * W4 / 4;
    constexpr int NW = kLkThreads / 64;
    static_assert((TK * W4) % 4 == 0 && (TK * NEED) % 4 == 0 && NEED >= 1 && NEED <= 4, "tile shape");
    static_assert(KPL % HS == 0 && V4 % HS == 0, "slices of whole keys");
    constexpr int SK = TK * W4 / HS, SO = TK * NEED;
    constexpr int SKR = STG ? 2 * SK : SK;  // STG 1 / 2: two slice buffers
    static_assert(STG == 0 || (SK * 4) % 1024 == 0, "DMA slices of whole 1-KB wave pieces");
    __shared__ __attribute__((aligned(16))) uint32_t lds[SKR > SO ? SKR : SO];
    constexpr uint32_t AG = kLkAG;
    __shared__ uint32_t ag[NW][3][AG];  // per-wave second-window list: start, K, kk | bc << 12 | search << 16
    __shared__ uint32_t nslow_tile;
    uint32_t* const sk = lds;
    uint32_t* const so = lds;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const LkStages<NEED, 12> lk(cv);
    static_assert(TK <= (1 << 12), "a tile slot is 12 bits of a list word");
#ifdef RP_LK_PROF
    uint64_t pa[6] = {0, 0, 0, 0, 0, 0}, ntl = 0;
#endif
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * TK;
        uint32_t h[KPL];
        LK_T(t0, tid);
        if constexpr (STG == 1 || STG == 2) {
            // DMA ring: slice s in buffer s & 1; a slice is SLI 1-KB wave pieces dealt over the
            // waves (wave w takes pieces w, w + NW, ...), so wave w waits for its own pieces of
            // slice s with a counted vmcnt (its pieces of slice s + 1 may stay in flight), then
            // the workgroup barrier makes every wave's pieces visible
            constexpr int SLB = SK * 4, SLI = SLB / 1024, PW = SLI / NW, PX = SLI % NW;
            const uint8_t* src = keys + base * LEN;
            uint8_t* ring = reinterpret_cast<uint8_t*>(lds);
            auto dma = [&](int sl) {
#pragma unroll
                for (int i = 0; i < PW + 1; i++)
                    if (i < PW || wv < PX) {
                        const void* g = reinterpret_cast<const void*>(src + sl * SLB + (i * NW + wv) * 1024 + lane * 16);
                        uint8_t* l = ring + (sl & 1) * SLB + (i * NW + wv) * 1024;
                        if constexpr (STG == 1) {
                            __builtin_amdgcn_global_load_lds(g, l, 16, 0, 0);
                        } else {
                            // the same DMA in asm: the compiler does not see an LDS write in flight,
                            // so it does not drain vmcnt(0) before the next slice's ds_reads (the
                            // counted waits below order them)
                            const uint32_t lo = __builtin_amdgcn_readfirstlane(
                                (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)l);
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // m0 is set here; the kernel has no other m0 use
                            asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
                                         :
                                         : "v"(g), "s"(lo)
                                         : "memory", "m0");
#pragma clang diagnostic pop
                        }
                    }
            };
            if (tid == 0) nslow_tile = 0;
            dma(0);
            if (HS > 1) dma(1);
#pragma unroll
            for (int hs = 0; hs < HS; hs++) {
                if (hs + 1 < HS) {
                    if (wv < PX)
                        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PW + 1) : "memory");
                    else
                        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PW) : "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
#ifdef RP_LK_PROF
                if (hs == 0) {
                    LK_T(tk, lds[tid]);
                    pa[0] += tk - t0;
                }
#endif
                const uint32_t* sb = lds + (hs & 1) * SK;
#pragma unroll
                for (int k = hs * (KPL / HS); k < (hs + 1) * (KPL / HS); k++) {
                    uint32_t w[W4];
#pragma unroll
                    for (int j = 0; j < W4; j++) w[j] = sb[(tid + (k - hs * (KPL / HS)) * kLkThreads) * W4 + j];
                    h[k] = fh::hash32_words<LEN>(w);
                }
                if (hs + 2 < HS) {  // this buffer is free once every wave has hashed from it
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                    dma(hs + 2);
                }
            }
        } else {
            lk_key_stage<kLkThreads, KPL, HS>(
                keys + base * LEN, sk, tid, h, [&] { if (tid == 0) nslow_tile = 0; },
                [&] {
#ifdef RP_LK_PROF
                    LK_T(tk, sk[tid]);
                    pa[0] += tk - t0;
#endif
                });
        }
        LK_T(t2, h[KPL - 1]);
        __syncthreads();  // sk is reused as so below
        uint32_t nag = 0;  // wave-uniform length of this wave's list
        uint8_t* const cnt_tile = counts ? counts + base : nullptr;
        auto defer = [&](uint32_t kk) {  // to the tile's list, for the exact fix path
            const uint32_t sp = atomicAdd(&nslow_tile, 1u);
            if (sp < kSlowPerTile) slow_list[t * kSlowPerTile + sp] = kk;
        };
        // LH > 1: the index and window trips run for KPL / LH keys at a time (fewer live
        // registers in this phase; A/B: RP_LOOKUP_LH)
        constexpr int KH = KPL / LH;
        static_assert(KPL % LH == 0, "whole halves");
#ifdef RP_LK_PROF
        uint64_t t3 = 0;
#endif
#pragma unroll
        for (int hh = 0; hh < LH; hh++) {
        if (hh) __builtin_amdgcn_sched_barrier(0);
        u32x2 rec[KH];
#pragma unroll
        for (int kq = 0; kq < KH; kq++) rec[kq] = lk.index_rec(h[hh * KH + kq]);
        uint32_t lo[KH], bc[KH], ws[KH];
        u32x4 win[KH];
#pragma unroll
        for (int kq = 0; kq < KH; kq++) win[kq] = lk.window(h[hh * KH + kq], rec[kq], lo[kq], bc[kq], ws[kq]);
#ifdef RP_LK_PROF
        if (hh == 0) {
            LK_T(t3h, lo[KH - 1]);
            t3 = t3h;
        }
#endif
#pragma unroll
        for (int kq = 0; kq < KH; kq++) {
            const int k = hh * KH + kq;
            lk.resolve(win[kq], h[k], lo[kq], bc[kq], ws[kq], (uint32_t)(tid + k * kLkThreads), nag, ag[wv], so, cnt_tile,
                       defer);
        }
        }  // halves
        LK_T(t4, nag);
        // second windows, one listed key per lane (the list is this wave's own LDS rows)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (uint32_t j = lane; j < (nag < AG ? nag : AG); j += 64)
            lk.finish2(lk.load16(ag[wv][0][j]), ag[wv][1][j], ag[wv][2][j], so, cnt_tile, defer);
        LK_T(t5a, nag);
        __syncthreads();
        LK_T(t5, tid);
        if (tid == 0) slow_cnt[t] = nslow_tile;
        u32x4* d4 = reinterpret_cast<u32x4*>(out + base * NEED);
        const u32x4* s4 = reinterpret_cast<const u32x4*>(so);
#pragma unroll
        for (int k = tid; k < TK * NEED / 4; k += kLkThreads) __builtin_nontemporal_store(s4[k], d4 + k);
        __syncthreads();
#ifdef RP_LK_PROF
        LK_T(t6, tid);
        pa[1] += t2 - t0;
        pa[2] += t3 - t2;
        pa[3] += t4 - t3;
        pa[4] += t5a - t4;
        pa[5] += t6 - t5;
        ntl += 1;
        (void)t5;
#endif
    }
#ifdef RP_LK_PROF
    if (lane == 0) {
        for (int i = 0; i < 6; i++) atomicAdd(&g_lk_prof[i], (unsigned long long)pa[i]);
        atomicAdd(&g_lk_prof[6], (unsigned long long)ntl);
    }
#endif
    if constexpr (FUSE) {
        // this workgroup's tiles t = blockIdx.x + i * gridDim.x; their rows are stored (the barrier
        // above orders the overwrites after them)
        constexpr uint32_t TPP = kLkThreads / kSlowPerTile;
        const uint64_t nt = ntiles > blockIdx.x ? (ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
        for (uint64_t i0 = 0; i0 < nt; i0 += TPP) {
            const uint64_t i = i0 + (uint32_t)tid / kSlowPerTile;
            const uint32_t q = (uint32_t)tid % kSlowPerTile;
            if (i < nt) {
                const uint64_t t = blockIdx.x + i * gridDim.x;
                const uint32_t c = slow_cnt[t];
                if (c <= kSlowPerTile) {
                    if (q < c) lookupn_redo(keys, fv, np, (uint32_t)NEED, out, counts, t * TK + slow_list[t * kSlowPerTile + q]);
                } else {
                    for (uint32_t k = q; k < (uint32_t)TK; k += kSlowPerTile) lookupn_redo(keys, fv, np, (uint32_t)NEED, out, counts, t * TK + k);
                }
            }
        }
    }
}

// ---- The sorted-tile lean kernel (the C2 default at 256 threads; RP_LOOKUP_SORT = 0 | 256 | 512 |
// 1024 threads). The lean
// kernel's index load holds 64 unrelated hashes per wave instruction, so every lane costs an
// L1 -> L2 request. Here a tile of 8 * THREADS keys is ordered by its top hash bits with a
// counting sort in LDS before the trips, and the ordered slots are dealt to lanes so that one
// wave instruction holds 64 consecutive slots: neighbouring lanes share index lines (4,096
// 128-B lines of 8-B group records at C2) and sometimes window lines
// (tools/model_sorted_lines.py). Only which 64 keys share an instruction matters, not their
// order inside it, so THREADS bins (8 keys a bin, 8 bins an instruction; the same shift for
// every ring) share within 0.02 requests a key of what 4,096 bins do, and their counters are
// scanned by one wave (4,096 bins, first built: 0.900 against 0.878 ms for the lean kernel).
// Everything per key is the lean kernel's (LkStages); rows are addressed by the key's tile slot
// kk, so results, counts and the deferred set do not depend on the order. Deferred keys go to
// the lean kernel's 2,048-key logical tiles (list tile * TK / 2048 + kk / 2048, slot kk % 2048),
// so k_lookupn_fix_tiles runs unchanged. Workgroups only meet at __syncthreads.
// LDS: rows (12 B a key) over the key slice (<= 18 KB per 256 threads) and the ordered (h, kk)
// pairs (8 B a key), both dead before the rows are written; + the 16-bit bin counters (two to
// a word) and the per-wave lists.
//
// Two kernels run the same tile body. Strided (k_lookupn_sorted): workgroup b takes tiles b,
// b + grid, ... Ticketed (k_lookupn_sorted_ticket, launched at 256 threads; RP_LOOKUP_TICKET):
// the strided kernel's body with the marked additions, as a kernel of its own because the body
// moved into a function both inline is scheduled differently by the compiler, and the strided
// kernels' code is to stay what was measured (tools/cmp_device_asm.py). There
// the grid is what is resident; a workgroup starts on tile blockIdx.x and draws every later one,
// grid + a ticket, from the device counter tick[0]. Lane 0 draws with one relaxed agent-scope
// atomicAdd at the top of the tile before, keeps the ticket in a register under that tile's key
// stream, hands it to the other lanes through LDS across barriers the loop has anyway, and a tile
// index >= ntiles ends the workgroup before anything is written for it. No wave ever waits on
// another workgroup, so the launch drains however few workgroups are resident. tick[1] counts
// the workgroups that have left: the last one puts both words back to 0 (every draw of every
// workgroup has returned by then), so a call costs no memset and no extra launch.
// Stagger (RP_LOOKUP_STAGGER): before its first tile the workgroup in resident slot
// j = (blockIdx.x / slot_div) % 4 of its CU sleeps j * stagger s_sleep(16) (a count fixed at
// launch, never a wait on memory), so a CU's workgroups do not run their phases in step.
#ifdef RP_LK_PROF
__device__ unsigned long long g_sk_prof[10];
#define RP_LK_TL
#endif
// -DRP_LK_TL alone: the timeline without the phase counters, whose waits slow the kernel by a fifth.
#ifdef RP_LK_TL
// The launch's timeline (tools/lk_timeline.py; s_memrealtime, 100 MHz): per workgroup its start
// and end stamps and HW_ID / XCC_ID, per tile its end stamp and workgroup. Nothing reads these
// on the device.
constexpr uint32_t kTlMaxWg = 16384, kTlMaxTiles = 32768;
__device__ unsigned long long g_tl_wg[2 * kTlMaxWg];
__device__ uint32_t g_tl_hw[2 * kTlMaxWg];
__device__ unsigned long long g_tl_tile[kTlMaxTiles];
__device__ uint32_t g_tl_tile_wg[kTlMaxTiles];
#define RP_TL_BEGIN()                                                                  \
    if (threadIdx.x == 0 && blockIdx.x < kTlMaxWg) {                                   \
        g_tl_wg[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();                    \
        g_tl_hw[2 * blockIdx.x] = __builtin_amdgcn_s_getreg(4 | (31 << 11));      /* HW_ID */  \
        g_tl_hw[2 * blockIdx.x + 1] = __builtin_amdgcn_s_getreg(20 | (31 << 11)); /* XCC_ID */ \
    }
#define RP_TL_TILE(t)                                      \
    if (threadIdx.x == 0 && (t) < kTlMaxTiles) {           \
        g_tl_tile[t] = __builtin_amdgcn_s_memrealtime();   \
        g_tl_tile_wg[t] = blockIdx.x;                      \
    }
#define RP_TL_END() \
    if (threadIdx.x == 0 && blockIdx.x < kTlMaxWg) g_tl_wg[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime()
#else
#define RP_TL_BEGIN()
#define RP_TL_TILE(t)
#define RP_TL_END()
#endif
constexpr int kSortDefault = 256;  // RP_LOOKUP_SORT when unset (0: the lean kernel; profiles/LOG.md)
constexpr bool kTicketDefault = true;   // RP_LOOKUP_TICKET when unset (0.810 against 0.834 ms strided; profiles/LOG.md)
constexpr int kStaggerDefault = 0;      // RP_LOOKUP_STAGGER when unset, sixteenths of a tile time (1/8, 1/4: no gain; 1/2: slower)
constexpr uint64_t kSortedTileUs = 25;  // a 2,048-key tile of a resident workgroup at C2 (0.2 ms / 8 tiles)
constexpr uint32_t kStaggerSlots = 4;   // resident workgroups a CU the stagger tells apart

template <int THREADS, int NEED>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4))) void k_lookupn_sorted(
    const uint8_t* __restrict__ keys, uint64_t ntiles, CompactView cv, uint32_t* __restrict__ out,
    uint8_t* __restrict__ counts, uint32_t* __restrict__ slow_list, uint32_t* __restrict__ slow_cnt) {
    constexpr int LEN = 36, W4 = LEN / 4, KPL = 8, HS = 4;
    constexpr int TK = THREADS * KPL;
    constexpr int NW = THREADS / 64;
    constexpr int SUB = TK / 2048;  // the lean kernel's logical tiles in one of these
    constexpr int SK = TK * W4 / HS, SO = TK * NEED;
    constexpr int BINS = THREADS;                 // 256 | 512 | 1024 bins on the top hash bits
    constexpr int BSH = 32 - (BINS == 256 ? 8 : BINS == 512 ? 9 : 10);
    constexpr int CW = BINS / 2;                  // counter words: two 16-bit bins each
    constexpr int WPL = CW / 64;                  // counter words a lane of the scanning wave takes
    static_assert(THREADS == 256 || THREADS == 512 || THREADS == 1024, "whole 2,048-key logical tiles, 13-bit slots, 16-bit bin counters");
    static_assert(2 * TK <= SO && SK <= SO, "the ordered pairs and the key slice fit under the rows");
    __shared__ __attribute__((aligned(16))) uint32_t lds[SO];
    __shared__ uint32_t ag[NW][3][kLkAG];  // per-wave second-window list (LkStages::resolve)
    __shared__ uint32_t bins[CW];
    __shared__ uint32_t nslow_sub[SUB];
    uint32_t* const sk = lds;  // a slice of 128 keys a wave
    uint32_t* const so = lds;
    u32x2* const pairs = reinterpret_cast<u32x2*>(lds);  // TK x (h, kk)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const LkStages<NEED, 13> lk(cv);
#ifdef RP_LK_PROF
    uint64_t pa[6] = {0, 0, 0, 0, 0, 0}, ntl = 0;
#endif
    RP_TL_BEGIN();
    if (tid < CW) bins[tid] = 0;
    if (tid < SUB) nslow_sub[tid] = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * TK;
        uint32_t h[KPL], kk[KPL];
        LK_T(t0, tid);
        // each wave stages and hashes its own 512 keys (tile slots wv * 512 + lane + 64 k): no
        // workgroup barrier until the counts
        lk_key_stage<64, KPL, HS, true>(keys + (base + (uint64_t)wv * 512) * LEN, sk + wv * (SK / NW), lane, h, [] {}, [] {});
        LK_T(t1, h[KPL - 1]);
        // rank in the bin: one LDS atomic per key (its half of the counter word)
        uint32_t rank[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const uint32_t b = h[k] >> BSH, sh = (b & 1u) * 16u;
            rank[k] = (atomicAdd(&bins[b >> 1], 1u << sh) >> sh) & 0xFFFFu;
        }
        __syncthreads();  // the counts are whole, and the last key slice is hashed
        if (wv == 0) {  // exclusive scan of the bin counts in place, by one wave: bin starts
            uint32_t c[WPL], sum = 0;
#pragma unroll
            for (int i = 0; i < WPL; i++) {
                c[i] = bins[lane * WPL + i];
                sum += (c[i] & 0xFFFFu) + (c[i] >> 16);
            }
            uint32_t x = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(x, o, 64);
                if (lane >= o) x += y;
            }
            uint32_t run = x - sum;
#pragma unroll
            for (int i = 0; i < WPL; i++) {
                const uint32_t a = run, b = run + (c[i] & 0xFFFFu);
                run = b + (c[i] >> 16);
                bins[lane * WPL + i] = a | (b << 16);  // starts <= TK <= 8192
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const uint32_t b = h[k] >> BSH, sh = (b & 1u) * 16u;
            const uint32_t slot = ((bins[b >> 1] >> sh) & 0xFFFFu) + rank[k];
            pairs[slot] = u32x2{h[k], (uint32_t)(wv * 512 + lane + 64 * k)};
        }
        __syncthreads();
        // lane tid takes slots tid + k THREADS: a wave instruction holds 64 consecutive slots
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const u32x2 p = pairs[tid + k * THREADS];
            h[k] = p.x;
            kk[k] = p.y;
        }
        if (tid < CW) bins[tid] = 0;  // for the next tile (the starts were read before the barrier above)
        if (tid < SUB) nslow_sub[tid] = 0;
        LK_T(t2, kk[KPL - 1]);
        __syncthreads();  // the pairs are dead: the rows take their place
        uint32_t nag = 0;  // wave-uniform length of this wave's list
        uint8_t* const cnt_tile = counts ? counts + base : nullptr;
        auto defer = [&](uint32_t k) {  // to the list of the key's 2,048-key logical tile
            const uint32_t s = k >> 11;
            const uint32_t sp = atomicAdd(&nslow_sub[s], 1u);
            if (sp < kSlowPerTile) slow_list[(t * SUB + s) * kSlowPerTile + sp] = k & 2047u;
        };
        u32x2 rec[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) rec[k] = lk.index_rec(h[k]);
        uint32_t lo[KPL], bc[KPL], ws[KPL];
        u32x4 win[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) win[k] = lk.window(h[k], rec[k], lo[k], bc[k], ws[k]);
        LK_T(t3, lo[KPL - 1]);
#pragma unroll
        for (int k = 0; k < KPL; k++) lk.resolve(win[k], h[k], lo[k], bc[k], ws[k], kk[k], nag, ag[wv], so, cnt_tile, defer);
        LK_T(t4, nag);
        // second windows, one listed key per lane (the list is this wave's own LDS rows)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (uint32_t j = lane; j < (nag < kLkAG ? nag : kLkAG); j += 64)
            lk.finish2(lk.load16(ag[wv][0][j]), ag[wv][1][j], ag[wv][2][j], so, cnt_tile, defer);
        LK_T(t5a, nag);
        __syncthreads();
        LK_T(t5, tid);
        if (tid < SUB) slow_cnt[t * SUB + tid] = nslow_sub[tid];
        u32x4* d4 = reinterpret_cast<u32x4*>(out + base * NEED);
        const u32x4* s4 = reinterpret_cast<const u32x4*>(so);
#pragma unroll
        for (int k = tid; k < TK * NEED / 4; k += THREADS) __builtin_nontemporal_store(s4[k], d4 + k);
        __syncthreads();
#ifdef RP_LK_PROF
        LK_T(t6, tid);
        pa[0] += t1 - t0;
        pa[1] += t2 - t1;
        pa[2] += t3 - t2;
        pa[3] += t4 - t3;
        pa[4] += t5a - t4;
        pa[5] += t6 - t5;
        ntl += 1;
#endif
        RP_TL_TILE(t);
    }
#ifdef RP_LK_PROF
    if (lane == 0) {
        for (int i = 0; i < 6; i++) atomicAdd(&g_sk_prof[i], (unsigned long long)pa[i]);
        atomicAdd(&g_sk_prof[6], (unsigned long long)ntl);
    }
#endif
    RP_TL_END();
}

// The ticketed form (see above): k_lookupn_sorted's body, plus the stagger before the loop, the
// draw at the top of a tile, the hand-over of the ticket through next_tile, and the exit count.
// tick: Ring::tick. stagger: s_sleep(16) steps per resident slot (0: none). slot_div: blocks per
// resident slot (the CU count).
template <int THREADS, int NEED>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4))) void k_lookupn_sorted_ticket(
    const uint8_t* __restrict__ keys, uint64_t ntiles, CompactView cv, uint32_t* __restrict__ out,
    uint8_t* __restrict__ counts, uint32_t* __restrict__ slow_list, uint32_t* __restrict__ slow_cnt,
    uint32_t* __restrict__ tick, uint32_t stagger, uint32_t slot_div) {
    constexpr int LEN = 36, W4 = LEN / 4, KPL = 8, HS = 4;
    constexpr int TK = THREADS * KPL;
    constexpr int NW = THREADS / 64;
    constexpr int SUB = TK / 2048;  // the lean kernel's logical tiles in one of these
    constexpr int SK = TK * W4 / HS, SO = TK * NEED;
    constexpr int BINS = THREADS;                 // 256 | 512 | 1024 bins on the top hash bits
    constexpr int BSH = 32 - (BINS == 256 ? 8 : BINS == 512 ? 9 : 10);
    constexpr int CW = BINS / 2;                  // counter words: two 16-bit bins each
    constexpr int WPL = CW / 64;                  // counter words a lane of the scanning wave takes
    static_assert(THREADS == 256 || THREADS == 512 || THREADS == 1024, "whole 2,048-key logical tiles, 13-bit slots, 16-bit bin counters");
    static_assert(2 * TK <= SO && SK <= SO, "the ordered pairs and the key slice fit under the rows");
    __shared__ __attribute__((aligned(16))) uint32_t lds[SO];
    __shared__ uint32_t ag[NW][3][kLkAG];  // per-wave second-window list (LkStages::resolve)
    __shared__ uint32_t bins[CW];
    __shared__ uint32_t nslow_sub[SUB];
    __shared__ uint32_t next_tile;  // the drawn ticket, from lane 0 to the workgroup
    uint32_t* const sk = lds;  // a slice of 128 keys a wave
    uint32_t* const so = lds;
    u32x2* const pairs = reinterpret_cast<u32x2*>(lds);  // TK x (h, kk)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const LkStages<NEED, 13> lk(cv);
#ifdef RP_LK_PROF
    uint64_t pa[6] = {0, 0, 0, 0, 0, 0}, ntl = 0;
#endif
    RP_TL_BEGIN();
    if (tid < CW) bins[tid] = 0;
    if (tid < SUB) nslow_sub[tid] = 0;
    const uint32_t naps = ((blockIdx.x / slot_div) % kStaggerSlots) * stagger;
    for (uint32_t i = 0; i < naps; i++) __builtin_amdgcn_s_sleep(16);
    uint64_t nxt = 0;
    uint32_t zero;
    asm("v_mov_b32 %0, 0" : "=v"(zero));
    for (uint64_t t = blockIdx.x; t < ntiles; t = nxt) {
        const uint64_t base = t * TK;
        uint32_t h[KPL], kk[KPL];
        // the next tile's ticket: the trip runs under this tile's key stream
        // (the zero the compiler cannot see keeps the address per-lane: with a uniform address
        // the add is rewritten as a wave-wide one whose result is broadcast, and waited for, here)
        uint32_t drawn = 0;
        if (tid == 0) drawn = __hip_atomic_fetch_add(tick + zero, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        LK_T(t0, tid);
        // each wave stages and hashes its own 512 keys (tile slots wv * 512 + lane + 64 k): no
        // workgroup barrier until the counts
        lk_key_stage<64, KPL, HS, true>(keys + (base + (uint64_t)wv * 512) * LEN, sk + wv * (SK / NW), lane, h, [] {}, [] {});
        LK_T(t1, h[KPL - 1]);
        // rank in the bin: one LDS atomic per key (its half of the counter word)
        uint32_t rank[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const uint32_t b = h[k] >> BSH, sh = (b & 1u) * 16u;
            rank[k] = (atomicAdd(&bins[b >> 1], 1u << sh) >> sh) & 0xFFFFu;
        }
        if (tid == 0) next_tile = drawn;  // read after the barrier that ends the trips below
        __syncthreads();  // the counts are whole, and the last key slice is hashed
        if (wv == 0) {  // exclusive scan of the bin counts in place, by one wave: bin starts
            uint32_t c[WPL], sum = 0;
#pragma unroll
            for (int i = 0; i < WPL; i++) {
                c[i] = bins[lane * WPL + i];
                sum += (c[i] & 0xFFFFu) + (c[i] >> 16);
            }
            uint32_t x = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(x, o, 64);
                if (lane >= o) x += y;
            }
            uint32_t run = x - sum;
#pragma unroll
            for (int i = 0; i < WPL; i++) {
                const uint32_t a = run, b = run + (c[i] & 0xFFFFu);
                run = b + (c[i] >> 16);
                bins[lane * WPL + i] = a | (b << 16);  // starts <= TK <= 8192
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const uint32_t b = h[k] >> BSH, sh = (b & 1u) * 16u;
            const uint32_t slot = ((bins[b >> 1] >> sh) & 0xFFFFu) + rank[k];
            pairs[slot] = u32x2{h[k], (uint32_t)(wv * 512 + lane + 64 * k)};
        }
        __syncthreads();
        // lane tid takes slots tid + k THREADS: a wave instruction holds 64 consecutive slots
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const u32x2 p = pairs[tid + k * THREADS];
            h[k] = p.x;
            kk[k] = p.y;
        }
        if (tid < CW) bins[tid] = 0;  // for the next tile (the starts were read before the barrier above)
        if (tid < SUB) nslow_sub[tid] = 0;
        LK_T(t2, kk[KPL - 1]);
        __syncthreads();  // the pairs are dead: the rows take their place
        uint32_t nag = 0;  // wave-uniform length of this wave's list
        uint8_t* const cnt_tile = counts ? counts + base : nullptr;
        auto defer = [&](uint32_t k) {  // to the list of the key's 2,048-key logical tile
            const uint32_t s = k >> 11;
            const uint32_t sp = atomicAdd(&nslow_sub[s], 1u);
            if (sp < kSlowPerTile) slow_list[(t * SUB + s) * kSlowPerTile + sp] = k & 2047u;
        };
        u32x2 rec[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) rec[k] = lk.index_rec(h[k]);
        uint32_t lo[KPL], bc[KPL], ws[KPL];
        u32x4 win[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) win[k] = lk.window(h[k], rec[k], lo[k], bc[k], ws[k]);
        LK_T(t3, lo[KPL - 1]);
#pragma unroll
        for (int k = 0; k < KPL; k++) lk.resolve(win[k], h[k], lo[k], bc[k], ws[k], kk[k], nag, ag[wv], so, cnt_tile, defer);
        LK_T(t4, nag);
        // second windows, one listed key per lane (the list is this wave's own LDS rows)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (uint32_t j = lane; j < (nag < kLkAG ? nag : kLkAG); j += 64)
            lk.finish2(lk.load16(ag[wv][0][j]), ag[wv][1][j], ag[wv][2][j], so, cnt_tile, defer);
        LK_T(t5a, nag);
        __syncthreads();
        LK_T(t5, tid);
        // (the word is next written before the next tile's first barrier, past the barrier below)
        nxt = (uint64_t)gridDim.x + next_tile;
        if (tid < SUB) slow_cnt[t * SUB + tid] = nslow_sub[tid];
        u32x4* d4 = reinterpret_cast<u32x4*>(out + base * NEED);
        const u32x4* s4 = reinterpret_cast<const u32x4*>(so);
#pragma unroll
        for (int k = tid; k < TK * NEED / 4; k += THREADS) __builtin_nontemporal_store(s4[k], d4 + k);
        __syncthreads();
#ifdef RP_LK_PROF
        LK_T(t6, tid);
        pa[0] += t1 - t0;
        pa[1] += t2 - t1;
        pa[2] += t3 - t2;
        pa[3] += t4 - t3;
        pa[4] += t5a - t4;
        pa[5] += t6 - t5;
        ntl += 1;
#endif
        RP_TL_TILE(t);
    }
#ifdef RP_LK_PROF
    if (lane == 0) {
        for (int i = 0; i < 6; i++) atomicAdd(&g_sk_prof[i], (unsigned long long)pa[i]);
        atomicAdd(&g_sk_prof[6], (unsigned long long)ntl);
    }
#endif
    RP_TL_END();
    // Lane 0's own last draw has returned (its value ended the loop), as has every draw of a
    // workgroup whose exit is counted: the workgroup that counts the last exit finds no draw in
    // flight and puts the two words back for the next launch.
    if (tid == 0) {
        const uint32_t left = __hip_atomic_fetch_add(tick + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (left + 1u == gridDim.x) {
            __hip_atomic_store(tick, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(tick + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- The wave-specialised lean kernel (round 6, A/B: RP_LOOKUP_WS). The lean kernel's waves run
// every phase in turn (key stream, hash, index trip, window trip, stores), and s_waitcnt vmcnt
// retires in issue order, so a wave cannot keep its next keys in flight behind its lookups. Here
// the NP producer waves of a workgroup only stream keys (16-B non-temporal loads, transposed
// through an 18-KB LDS tile per producer, the next tile's loads in flight) and hash them into an
// LDS ring (slots of 512 hashes), and the NC consumer waves only take the index and window trips
// and store the rows (a 12-B
// buffer store per key: 768 contiguous bytes per wave instruction; second-window keys' rows
// from the lane that finishes them). Producer p serves consumers p, p + NP, ...; the ring's
// counters are LDS words (prod[c]: wave-tiles filled, cons[c]: wave-tiles read). Every wait is
// bounded (kWsSpin polls): past it the wave stops waiting and sets *err, so the grid always
// drains (the launch's results are then wrong; the launcher reports it under RP_LOOKUP_DEBUG).
// Deferred keys go to per-wave-tile lists (k_lookupn_fix_tiles with TK 512).
// Measured (profiles/r06/r06at-r06aw): 1.10 ms per 2^26 C2 keys at 4:12 against the lean kernel's
// 0.88; alone, the producers take 0.58 ms and the consumers 0.68, and split this way the two add
// up (both move their bytes through the L2 -> CU return path). The lean kernel stays the default.
constexpr int kWsSlots = 2;
constexpr uint32_t kWsSpin = 1u << 22;
typedef uint32_t u32x3v __attribute__((ext_vector_type(3)));

// ABL (diagnostics, RP_LOOKUP_WS_ABL; results wrong, times only): 1 = producers load no keys (the
// hashes are made from the key index), 2 = consumers take no trips (the row is the hash).
template <int NP, int NC, int ABL = 0>
__global__ __launch_bounds__((NP + NC) * 64) __attribute__((amdgpu_waves_per_eu(4))) void k_lookupn_ws(const uint8_t* __restrict__ keys, uint64_t nwt,
                                                               CompactView cv, uint32_t* __restrict__ out,
                                                               uint32_t out_bytes, uint8_t* __restrict__ counts,
                                                               uint32_t* __restrict__ slow_list,
                                                               uint32_t* __restrict__ slow_cnt,
                                                               uint32_t* __restrict__ err) {
    constexpr int NEED = 3, KPL = 8, LEN = 36, W4 = LEN / 4;
    constexpr int TK = 64 * KPL;         // keys a wave-tile
    constexpr int V4 = TK * W4 / 4;      // its 16-B pieces
    constexpr int PER = V4 / 64;         // per producer lane
    constexpr uint32_t SPAN = 5 - NEED;
    constexpr uint32_t AG = 64;
    static_assert(V4 % 64 == 0, "wave-tile shape");
    __shared__ __attribute__((aligned(16))) uint32_t stg[NP][V4 * 4];
    __shared__ uint32_t ring[NC][kWsSlots][TK];
    __shared__ uint32_t ag[NC][3][AG];
    __shared__ uint32_t prod[NC], cons[NC], nsl[NC];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < NC) {
        prod[tid] = 0;
        cons[tid] = 0;
    }
    __syncthreads();
    const uint64_t nwg = (nwt + NC - 1) / NC;  // workgroup tiles: NC wave-tiles each
    // until *p >= target (wave-uniform: one LDS word read by the whole wave)
    auto wait_ge = [&](uint32_t* p, uint32_t target) {
        for (uint32_t n = 0;; n++) {
            const uint32_t v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
            if (v >= target) break;
            if (n == kWsSpin) {
                if (lane == 0) atomicOr(err, 1u);
                break;
            }
            __builtin_amdgcn_s_sleep(1);
            asm volatile("" ::: "memory");
        }
        asm volatile("" ::: "memory");
    };
    if (wv < NP) {
        // producer: item j is consumer c = wv + (j % cnt) NP's wave-tile of workgroup tile
        // blockIdx.x + (j / cnt) gridDim.x (ring sequence j / cnt). The whole wave-tile's keys go
        // to LDS at once, and the next item's 18 loads a lane are issued before this one is
        // hashed, so the key stream stays in flight behind the hashing and the ring waits.
        const int cnt = (NC - wv + NP - 1) / NP;
        auto item_wt = [&](uint32_t j) -> uint64_t {
            const uint64_t T = blockIdx.x + (uint64_t)(j / cnt) * gridDim.x;
            const uint64_t wt = T * NC + wv + (j % cnt) * NP;
            return T < nwg && wt < nwt ? wt : ~0ull;
        };
        u32x4 pre[PER];
        auto issue = [&](uint64_t wt) {
            const u32x4* s4 = reinterpret_cast<const u32x4*>(keys + wt * (uint64_t)(TK * LEN));
#pragma unroll
            for (int q = 0; q < PER; q++) pre[q] = __builtin_nontemporal_load(s4 + lane + 64 * q);
        };
        uint64_t wt = item_wt(0);
        if (ABL != 1 && wt != ~0ull) issue(wt);
        for (uint32_t j = 0; wt != ~0ull; j++) {
            const uint64_t wn = item_wt(j + 1);
            uint32_t h[KPL];
            if constexpr (ABL == 1) {
#pragma unroll
                for (int k = 0; k < KPL; k++) h[k] = (uint32_t)(wt * TK + lane + 64 * k) * 0x9E3779B1u;
            } else {
                u32x4* st4 = reinterpret_cast<u32x4*>(stg[wv]);
#pragma unroll
                for (int q = 0; q < PER; q++) st4[lane + 64 * q] = pre[q];
                __builtin_amdgcn_wave_barrier();
                if (wn != ~0ull) issue(wn);
#pragma unroll
                for (int k = 0; k < KPL; k++) {
                    uint32_t w[W4];
#pragma unroll
                    for (int x = 0; x < W4; x++) w[x] = stg[wv][(lane + 64 * k) * W4 + x];
                    h[k] = fh::hash32_words<LEN>(w);
                }
            }
            __builtin_amdgcn_wave_barrier();
            const int c = wv + (int)(j % cnt) * NP;
            const uint32_t i = j / cnt;
            wait_ge(&cons[c], i + 1 > (uint32_t)kWsSlots ? i + 1 - kWsSlots : 0u);
            uint32_t* slot = ring[c][i % kWsSlots];
#pragma unroll
            for (int k = 0; k < KPL; k++) slot[lane + 64 * k] = h[k];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) __hip_atomic_store(&prod[c], i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            wt = wn;
        }
        return;
    }
    // consumer c: its wave-tile of every workgroup tile
    const int c = wv - NP;
    const uint32_t omask = (1u << cv.ob) - 1u, obit = 1u << cv.ob;
    const uint32_t bsh = 32u - cv.cb;
    const uint32_t rmask = (1u << bsh) - 1u;
    const __amdgpu_buffer_rsrc_t ent_r =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(cv.ent), 0, (int)cv.ent_bytes, 0x00020000);
    const bool hinted = cv.idxh != nullptr;
    const __amdgpu_buffer_rsrc_t idx_r = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint32_t*>(hinted ? cv.idxh : cv.idx), 0, (int)cv.idx_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t out_r = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)out_bytes, 0x00020000);
    auto load16 = [&](uint32_t pos) {
        return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ent_r, (int)(3u * pos), 0, 0));
    };
    auto ent5v = [&](const u32x4 v, uint32_t (&e)[5]) {
        e[0] = v.x & 0xFFFFFFu;
        e[1] = (v.x >> 24) | ((v.y & 0xFFFFu) << 8);
        e[2] = (v.y >> 16) | ((v.z & 0xFFu) << 16);
        e[3] = v.z >> 8;
        e[4] = v.w & 0xFFFFFFu;
    };
    auto wstart = [&](uint32_t hk, uint32_t bck, uint32_t hint) -> uint32_t {
        const int fl = (int)((((hk << cv.cb) >> 24) * bck) >> 8) - 2 + (int)hint;
        return (cv.wpred && bck <= 10u && fl > 0) ? (uint32_t)fl : 0u;
    };
    auto store_row = [&](uint64_t key, uint32_t a, uint32_t b, uint32_t d) {
        const u32x3v v = {a, b, d};
        __builtin_amdgcn_raw_buffer_store_b96(v, out_r, (int)(key * 12u), 0, 2);
    };
    uint32_t i = 0;
    for (uint64_t T = blockIdx.x; T < nwg; T += gridDim.x, i++) {
        const uint64_t wt = T * NC + c;
        if (wt >= nwt) break;
        const uint64_t base = wt * TK;
        wait_ge(&prod[c], i + 1);
        uint32_t h[KPL];
        const uint32_t* slot = ring[c][i % kWsSlots];
#pragma unroll
        for (int k = 0; k < KPL; k++) h[k] = slot[lane + 64 * k];
        if (lane == 0) nsl[c] = 0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(&cons[c], i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if constexpr (ABL == 2) {
#pragma unroll
            for (int k = 0; k < KPL; k++) store_row(base + lane + 64 * k, h[k], h[k] + 1u, h[k] + 2u);
            if (lane == 0) slow_cnt[wt] = 0;
            continue;
        }
        u32x2 rec[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++)
            rec[k] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(idx_r, (int)((h[k] >> (bsh + 3u)) * 8u), 0, 0));
        uint32_t lo[KPL], bc[KPL], ws[KPL];
        u32x4 win[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const uint32_t s4 = ((h[k] >> bsh) & 7u) * 4u;
            const uint32_t below = rec[k].y & ((1u << s4) - 1u);
            uint32_t b0 = rec[k].x, hint = 1u;
            if (hinted) {
                const uint32_t g = h[k] >> (bsh + 3u);
                b0 = (uint32_t)(((uint64_t)g * cv.M) >> (cv.cb - 3u)) + (uint32_t)((int32_t)(rec[k].x << 18) >> 18);
                hint = (rec[k].x >> (14u + (s4 >> 1))) & 3u;
            }
            lo[k] = b0 + __builtin_amdgcn_sad_u8(below & 0x0F0F0F0Fu, 0u, __builtin_amdgcn_sad_u8((below >> 4) & 0x0F0F0F0Fu, 0u, 0u));
            bc[k] = (rec[k].y >> s4) & 15u;
            ws[k] = wstart(h[k], bc[k], hint);
            win[k] = load16(lo[k] + ws[k]);
        }
        uint32_t nag = 0;
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            uint32_t e[5];
            ent5v(win[k], e);
            const uint32_t K = ((h[k] & rmask) >> cv.fsh) << cv.ob;
            const uint32_t w = ws[k];
            uint32_t lt = 0;
            bool tie = false;
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const bool inb = (uint32_t)j + w < bc[k];
                lt += (inb && e[j] < K);
                tie |= (inb && e[j] - K < obit);
            }
            uint32_t r[NEED];
#pragma unroll
            for (int q = 0; q < NEED; q++) {
                uint32_t v = e[q] & omask;
#pragma unroll
                for (uint32_t d = 1; d <= SPAN; d++) v = lt == d ? (e[q + d] & omask) : v;
                r[q] = v;
            }
            const bool dup = r[0] == r[1] || r[0] == r[2] || r[1] == r[2];
            const uint32_t kk = lane + 64 * k;
            bool slow = (tie && !cv.exact) | (lo[k] + 20u > cv.M);
            const bool under = w > 0u && lt == 0u;
            const bool again = !slow && (lt > SPAN || dup || under);
            const uint64_t m = __ballot(again);
            const uint32_t pos = nag + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            nag += (uint32_t)__popcll(m);
            if (again) {
                if (pos < AG) {
                    const uint32_t b0 = under ? (w > 2u ? w - 2u : 0u) : w + 5u;
                    const bool search = under || (lt == 5u && bc[k] > w + 5u);
                    ag[c][0][pos] = lo[k] + (search ? b0 : w + lt);
                    ag[c][1][pos] = K;
                    ag[c][2][pos] = kk | (bc[k] << 12) | ((uint32_t)search << 16) | ((search ? b0 : 0u) << 17) |
                                    ((uint32_t)(under && b0 > 0u) << 21);
                } else {
                    slow = true;
                }
            }
            if (!again || pos >= AG) {
                store_row(base + kk, r[0], r[1], r[2]);
                if (counts) counts[base + kk] = (uint8_t)NEED;
            }
            if (slow) {
                const uint32_t sp = atomicAdd(&nsl[c], 1u);
                if (sp < kSlowPerTile) slow_list[wt * kSlowPerTile + sp] = kk;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (uint32_t j = lane; j < (nag < AG ? nag : AG); j += 64) {
            const u32x4 wn = load16(ag[c][0][j]);
            const uint32_t K = ag[c][1][j], w2 = ag[c][2][j];
            const uint32_t kk = w2 & 0xFFFu, bck = (w2 >> 12) & 15u, b0 = (w2 >> 17) & 15u;
            uint32_t e2[5];
            ent5v(wn, e2);
            uint32_t off = 0;
            bool slow = false;
            if ((w2 >> 16) & 1u) {
                bool tie = false;
#pragma unroll
                for (int j2 = 0; j2 < 5; j2++) {
                    const bool inb = (uint32_t)j2 + b0 < bck;
                    off += (inb && e2[j2] < K);
                    tie |= (inb && e2[j2] - K < obit);
                }
                slow = (tie && !cv.exact) | (off == 5u && bck > b0 + 5u) | (((w2 >> 21) & 1u) && off == 0u);
            }
            uint32_t res[4] = {NIL, NIL, NIL, NIL};
            const uint32_t rc = dedupe5(e2, off, omask, NEED, res);
            slow |= rc < (uint32_t)NEED;
            if (slow) {
                const uint32_t sp = atomicAdd(&nsl[c], 1u);
                if (sp < kSlowPerTile) slow_list[wt * kSlowPerTile + sp] = kk;
            }
            store_row(base + kk, res[0], res[1], res[2]);
            if (counts) counts[base + kk] = (uint8_t)rc;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) slow_cnt[wt] = __hip_atomic_load(&nsl[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// ---- The LDS-index kernel (round 6). The lean kernel above takes two dependent L2 trips per key
// (the index record, then the window); its ablations price the index trip at 0.21 of 0.93 ms, and
// the access-pattern microbenchmark (profiles/r01c/ub_access_patterns.txt) puts one random 16-B
// load per key from a 3 MB table at 0.62 ms against 0.80 for two dependent ones. Here the index
// lives in LDS: one 768-thread workgroup per CU loads the NG group records (<= 128 KB, k_lidx_build)
// once, and each wave then streams its own tiles of 64 x KPL keys: 16-B non-temporal key loads,
// transposed through the wave's 2.3-KB LDS slice (one key per lane per slice) and hashed; the
// group record from LDS gives the bucket's first position and token count; the window is 10
// entries (32 B, two 16-B loads) from max(0, floor(u c) - 4) into the bucket (u: the key's place in
// the bucket's hash range), which holds the key's position and its NEED owners for all but ~0.45 %
// of C2 keys (a fingerprint tie: 0.43 %; a window that misses; a group with a bucket of 16+
// tokens; the ring end: the numpy emulation of the C2 ring in tools/emu_lds.py). Those
// are deferred to k_lookupn_fix_tiles (the exact tokens) through the per-tile lists, as in the
// compact kernels.
struct LdsView {
    const uint8_t* ent;  // 3 B per token (k_lpack3), M + kEnt3Pad + 6 entries (+16 B)
    const uint4* idx;    // ng group records (k_lidx_build)
    uint32_t M, ng, lg, fb, ob;
    uint32_t ent_bytes;
};
constexpr bool kLdsDefault = false;      // RP_LOOKUP_LDS=1 selects it (A/B)
constexpr int kLdsThreads = 768;          // 12 waves: one workgroup a CU (the index takes up to 128 KB)
constexpr uint32_t kLdsMaxGroups = 8192;  // 128 KB of group records

// STG 0: each lane loads its own keys (three loads per 36-B key: 16 + 16 + 4 B at a 36-B stride;
// the lines a wave touches are the same as the coalesced form's), no LDS transposition; STG 1:
// 16-B coalesced loads transposed through the wave's LDS slice (A/B: RP_LOOKUP_LDS_STG).
// ABL (diagnostics, RP_LOOKUP_LDS_ABL; results wrong, times only): 1 = no window loads (entries
// made from the group record), 2 = no LDS index read (a record made from the hash), 4 = rows not
// stored (one store of their xor per lane-tile).
template <int KPL, int NEED, int STG = 0, int ABL = 0>
__global__ __launch_bounds__(kLdsThreads) __attribute__((amdgpu_waves_per_eu(3))) void k_lookupn_lds(
    const uint8_t* __restrict__ keys, uint64_t nwt, LdsView lv, uint32_t* __restrict__ out,
    uint8_t* __restrict__ counts, uint32_t* __restrict__ slow_list, uint32_t* __restrict__ slow_cnt) {
    constexpr int LEN = 36, W4 = LEN / 4, NWV = kLdsThreads / 64;
    constexpr int TK = 64 * KPL;       // keys per wave-tile
    constexpr int V4 = TK * W4 / 4;    // 16-B key vectors per wave-tile
    constexpr int PER = V4 / 64;       // per lane
    constexpr int SV = 64 * W4 / 4;    // vectors per slice of 64 keys
    static_assert(V4 % 64 == 0 && NEED >= 1 && NEED <= 4, "tile shape");
    __shared__ uint4 s_idx[kLdsMaxGroups];
    __shared__ __attribute__((aligned(16))) uint32_t s_key[STG ? NWV : 1][64 * W4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (uint32_t i = tid; i < lv.ng; i += kLdsThreads) s_idx[i] = lv.idx[i];
    __syncthreads();
    const uint32_t omask = (1u << lv.ob) - 1u, obit = 1u << lv.ob, lg = lv.lg, gsh = 32u - lv.lg;
    const uint32_t fsh = 32u - lv.fb;
    const __amdgpu_buffer_rsrc_t ent_r =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(lv.ent), 0, (int)lv.ent_bytes, 0x00020000);
    uint32_t* const sk = s_key[STG ? wv : 0];
    const uint64_t nwaves = (uint64_t)gridDim.x * NWV;
    auto nsum = [](uint32_t w, uint32_t acc) {  // the sum of w's eight nibbles, plus acc
        return __builtin_amdgcn_sad_u8(w & 0x0F0F0F0Fu, 0u, __builtin_amdgcn_sad_u8((w >> 4) & 0x0F0F0F0Fu, 0u, acc));
    };
    for (uint64_t wt = (uint64_t)blockIdx.x * NWV + wv; wt < nwt; wt += nwaves) {
        const uint64_t base = wt * TK;
        uint32_t h[KPL];
        if constexpr (STG == 0) {
            uint32_t kw[KPL][W4];
#pragma unroll
            for (int k = 0; k < KPL; k++) {
                const uint32_t* src = reinterpret_cast<const uint32_t*>(keys + (base + (uint64_t)k * 64 + lane) * LEN);
                const u32x4_a4 a = *reinterpret_cast<const u32x4_a4*>(src);
                const u32x4_a4 b = *reinterpret_cast<const u32x4_a4*>(src + 4);
                kw[k][0] = a.x; kw[k][1] = a.y; kw[k][2] = a.z; kw[k][3] = a.w;
                kw[k][4] = b.x; kw[k][5] = b.y; kw[k][6] = b.z; kw[k][7] = b.w;
                kw[k][8] = src[8];
            }
#pragma unroll
            for (int k = 0; k < KPL; k++) h[k] = fh::hash32_words<LEN>(kw[k]);
        } else {
        const u32x4* s4 = reinterpret_cast<const u32x4*>(keys + base * LEN);
        u32x4 pre[PER];
#pragma unroll
        for (int q = 0; q < PER; q++) pre[q] = __builtin_nontemporal_load(s4 + lane + 64 * q);
#pragma unroll
        for (int k = 0; k < KPL; k++) {  // slice k: keys k * 64 + lane, one per lane
#pragma unroll
            for (int q = 0; q < PER; q++) {
                const int v = (int)lane + 64 * q;
                if (v >= SV * k && v < SV * (k + 1)) reinterpret_cast<u32x4*>(sk)[v - SV * k] = pre[q];
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            uint32_t w[W4];
#pragma unroll
            for (int j = 0; j < W4; j++) w[j] = sk[lane * W4 + j];
            h[k] = fh::hash32_words<LEN>(w);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        }
        }  // STG
        // the group records (LDS), every key's window start, both window loads in flight
        uint32_t w0[KPL], bc[KPL], sw[KPL], K[KPL];
        bool gfull[KPL];
        u32x4 wa[KPL], wb[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const uint32_t x = h[k] << lg;
            const uint64_t t = (uint64_t)x * 28u;
            const uint32_t j = (uint32_t)(t >> 32), fr = (uint32_t)t, g = h[k] >> gsh;
            const uint4 rec = (ABL & 2) ? uint4{h[k] & 0x11111111u, h[k] & 0x22222222u, fr & 0x11111111u,
                                                (h[k] & 0x00FF1111u)}
                                        : s_idx[g];
            const uint32_t jb = 4u * j;  // the bucket's bit offset among the 112 count bits
            const uint32_t m0 = jb >= 32u ? ~0u : (1u << jb) - 1u;
            const uint32_t m1 = jb >= 64u ? ~0u : jb <= 32u ? 0u : (1u << (jb - 32u)) - 1u;
            const uint32_t m2 = jb >= 96u ? ~0u : jb <= 64u ? 0u : (1u << (jb - 64u)) - 1u;
            const uint32_t m3 = jb <= 96u ? 0u : (1u << (jb - 96u)) - 1u;
            const uint32_t below = nsum(rec.x & m0, nsum(rec.y & m1, nsum(rec.z & m2, nsum(rec.w & m3, 0u))));
            const uint32_t cw = jb < 32u ? rec.x : jb < 64u ? rec.y : jb < 96u ? rec.z : rec.w;
            const uint32_t c = (cw >> (jb & 31u)) & 15u;
            const uint32_t st = (uint32_t)(((uint64_t)g * lv.M) >> lg) + (uint32_t)((int32_t)rec.w >> 16) + below;
            const uint32_t fl = ((fr >> 24) * c) >> 8;  // about the key's position in the bucket
            const uint32_t s = fl > 4u ? fl - 4u : 0u;
            gfull[k] = (rec.w >> 16) == 0x8000u;
            w0[k] = gfull[k] ? 0u : st + s;
            sw[k] = s;
            bc[k] = c;
            K[k] = (fr >> fsh) << lv.ob;
            if constexpr ((ABL & 1) != 0) {
                wa[k] = u32x4{rec.x, rec.y, rec.z, w0[k]};
                wb[k] = u32x4{rec.w, K[k], fr, st};
            } else {
                wa[k] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ent_r, (int)(3u * w0[k]), 0, 0));
                wb[k] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ent_r, (int)(3u * w0[k] + 16u), 0, 0));
            }
        }
        uint32_t nsl = 0;  // wave-uniform: this wave-tile's deferred keys
        uint32_t sink = 0;
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const u32x4 a = wa[k], b = wb[k];
            const uint32_t e[10] = {a.x & 0xFFFFFFu,
                                    (a.x >> 24) | ((a.y & 0xFFFFu) << 8),
                                    (a.y >> 16) | ((a.z & 0xFFu) << 16),
                                    a.z >> 8,
                                    a.w & 0xFFFFFFu,
                                    (a.w >> 24) | ((b.x & 0xFFFFu) << 8),
                                    (b.x >> 16) | ((b.y & 0xFFu) << 16),
                                    b.y >> 8,
                                    b.z & 0xFFFFFFu,
                                    (b.z >> 24) | ((b.w & 0xFFFFu) << 8)};
            uint32_t lt = 0;  // in-bucket window entries below the key
            bool tie = false;
#pragma unroll
            for (int j = 0; j < 10; j++) {
                const bool inb = sw[k] + (uint32_t)j < bc[k];
                lt += (inb && e[j] < K[k]);
                tie |= (inb && e[j] - K[k] < obit);
            }
            uint32_t res[4] = {NIL, NIL, NIL, NIL}, rc = 0;
#pragma unroll
            for (int j = 0; j < 10; j++) {  // the first NEED distinct owners from the key's position
                const uint32_t o = e[j] & omask;
                const bool dup = (rc > 0 && o == res[0]) | (rc > 1 && o == res[1]) | (rc > 2 && o == res[2]);
                if ((uint32_t)j >= lt && !dup && rc < (uint32_t)NEED) {
                    res[0] = rc == 0 ? o : res[0];
                    res[1] = rc == 1 ? o : res[1];
                    res[2] = rc == 2 ? o : res[2];
                    res[3] = rc == 3 ? o : res[3];
                    rc++;
                }
            }
            // deferred: a tie, a group with a bucket of 16+ tokens, the key before the window (its guard entry
            // is not below it) or past it, owners not distinct inside it, the ring end
            const bool slow = tie | gfull[k] | (sw[k] > 0u && lt == 0u) | (lt == 10u) | (rc < (uint32_t)NEED) |
                              (w0[k] + 12u > lv.M);
            const uint32_t kk = (uint32_t)k * 64u + lane;
            uint32_t* row = out + (base + kk) * NEED;
            if constexpr ((ABL & 4) != 0) {
                sink ^= res[0] ^ res[1] ^ res[2] ^ res[3];
            } else {
#pragma unroll
                for (int q = 0; q < NEED; q++) __builtin_nontemporal_store(res[q], row + q);
                if (counts) counts[base + kk] = (uint8_t)NEED;
            }
            const uint64_t m = __ballot(slow);
            const uint32_t pos = nsl + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (slow && pos < kSlowPerTile) slow_list[wt * kSlowPerTile + pos] = kk;
            nsl += (uint32_t)__popcll(m);
        }
        if (lane == 0) slow_cnt[wt] = nsl;
        if constexpr ((ABL & 4) != 0) out[(base + lane) * NEED] = sink;
    }
}

// Exact completion of the keys the compact kernels deferred: one thread per list slot
// (kSlowPerTile per tile) redoes its key; the slots of a tile whose list overflowed share the
// whole tile. (One thread per tile, redoing its list serially, took 0.043 ms per C2 launch.)
template <class View>
__global__ __launch_bounds__(256) void k_lookupn_fix_tiles(const uint8_t* __restrict__ keys, View rv, int np,
                                                           uint32_t W, uint32_t* __restrict__ out,
                                                           uint8_t* __restrict__ counts,
                                                           const uint32_t* __restrict__ slow_list,
                                                           const uint32_t* __restrict__ slow_cnt, uint64_t ntiles,
                                                           uint32_t TK) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t t = gid / kSlowPerTile;
    const uint32_t q = (uint32_t)(gid % kSlowPerTile);
    if (t >= ntiles) return;
    // the count and the slot are independent loads (one trip); the slot is used only when q < count
    const uint32_t c = slow_cnt[t];
    const uint32_t kq = slow_list[t * kSlowPerTile + q];
    if (c == 0) return;
    auto redo = [&](uint64_t k) { lookupn_redo(keys, rv, np, W, out, counts, k); };
    if (c <= kSlowPerTile) {
        if (q < c) lookupn_redo(keys, rv, np, W, out, counts, t * TK + kq);
    } else {
        for (uint32_t k = q; k < TK; k += kSlowPerTile) redo(t * TK + k);
    }
}

// Exact completion of the keys k_lookupn_probe / k_lookupn_compact deferred (same stream, so it
// sees the list and overwrites those rows): binary search in the bucket + the reference walk.
template <int LEN, int MODE = 0, class View = PackedView>
__global__ __launch_bounds__(256) void k_lookupn_fix(const uint8_t* __restrict__ keys, View rv, int np,
                                                     uint32_t W, uint32_t* __restrict__ out,
                                                     uint8_t* __restrict__ counts,
                                                     const uint32_t* __restrict__ slow,
                                                     const uint32_t* __restrict__ nslow) {
    const uint32_t total = *nslow;
    const uint32_t gstride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < total; s += gstride) {
        const uint64_t k = slow[s];
        uint32_t w[LEN / 4];
        const uint32_t* src = reinterpret_cast<const uint32_t*>(keys + k * LEN);
#pragma unroll
        for (int j = 0; j < LEN / 4; j++) w[j] = src[j];
        const uint32_t h = fh::hash32_words<LEN>(w);
        const uint32_t i = rv.find(h);
        uint32_t res[4];
        int c;
        if constexpr (MODE == 2) {
            res[0] = i; res[1] = i + 1; res[2] = i + 2; res[3] = i + 3;
            c = 1;
        } else {
            c = ring_walk<4>(rv, i, np, res);
        }
        uint32_t* row = out + k * W;
#pragma unroll
        for (int q = 0; q < 4; q++)
            if ((uint32_t)q < W) row[q] = res[q];
        if (counts) counts[k] = (uint8_t)c;
    }
}

// Key k's hash as every pass over a key stream takes it: the caller's hash, else the bytes at
// k * stride, else the bytes at off[k] .. off[k + 1].
__device__ __forceinline__ uint32_t key_hash(const uint8_t* __restrict__ keys, const uint64_t* __restrict__ off,
                                             uint32_t stride, const uint32_t* __restrict__ hashes, uint64_t k) {
    if (hashes) return hashes[k];
    uint64_t b, e;
    if (stride) {
        b = k * stride;
        e = b + stride;
    } else {
        b = off[k];
        e = off[k + 1];
    }
    return fh::hash32(fh::PtrSrc{keys + b}, (uint32_t)(e - b));
}

// The hash of a 36-byte key from its nine dwords: in LDS (a staged tile's, k_moved / k_handoff) or
// in global memory at a 4-byte aligned address (k_route).
__device__ __forceinline__ uint32_t key_hash36(const uint32_t* src) {
    uint32_t w[9];
#pragma unroll
    for (int j = 0; j < 9; j++) w[j] = src[j];
    return fh::hash32_words<36>(w);
}

// Generic keys: per-thread byte fetches (variable length via uint64 offsets, or any stride),
// or precomputed hashes (hashes != null).
template <int MAXN, class View>
__global__ __launch_bounds__(kLkThreads) void k_lookupn_generic(const uint8_t* __restrict__ keys,
                                                                const uint64_t* __restrict__ off,
                                                                uint32_t stride,
                                                                const uint32_t* __restrict__ hashes,
                                                                uint64_t n, View rv, int np, uint32_t W,
                                                                uint32_t* __restrict__ out,
                                                                uint8_t* __restrict__ counts) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gstride) {
        const uint32_t i = rv.find(key_hash(keys, off, stride, hashes, k));
        uint32_t* row = out + k * W;
        int c;
        if constexpr (MAXN > 0) {
            uint32_t res[MAXN];
            c = ring_walk<MAXN>(rv, i, np, res);
#pragma unroll
            for (int q = 0; q < MAXN; q++)
                if ((uint32_t)q < W) row[q] = res[q];
            for (uint32_t q = MAXN; q < W; q++) row[q] = NIL;
        } else {
            c = ring_walk_global(rv, i, np, row, W);
        }
        if (counts) counts[k] = (uint8_t)(c > 255 ? 255 : c);
    }
}

// Small host batches (the drop-in's one-key lookup / lookupN calls, index.js:434-471): the keys
// travel in the kernel arguments and the rows go straight to pinned host memory, so a call is
// one launch and one stream sync instead of two copies each way (host_lookup).
constexpr uint32_t kSmallKeys = 64, kSmallBytes = 3072, kSmallW = 16;
struct SmallKeys {
    uint32_t n;
    uint16_t off[kSmallKeys + 1];
    uint8_t b[kSmallBytes];
};
template <int MAXN, class View>
__global__ __launch_bounds__(64) void k_lookupn_small(const SmallKeys sk, View rv, int np, uint32_t W,
                                                      uint32_t* __restrict__ out, uint8_t* __restrict__ counts) {
    __shared__ uint8_t kb[kSmallBytes];
    const uint32_t k = threadIdx.x, nb = sk.off[sk.n];
    for (uint32_t i = k; i < nb; i += 64) kb[i] = sk.b[i];
    __syncthreads();
    if (k >= sk.n) return;
    const uint32_t b = sk.off[k], e = sk.off[k + 1];
    const uint32_t i = rv.find(fh::hash32(fh::PtrSrc{kb + b}, e - b));
    uint32_t res[MAXN];
    const int c = ring_walk<MAXN>(rv, i, np, res);
    for (uint32_t q = 0; q < W; q++) out[k * W + q] = q < (uint32_t)MAXN ? res[q] : NIL;
    if (counts) counts[k] = (uint8_t)(c > 255 ? 255 : c);
}

// The lookup service (rp_ring_service): one resident wave answers single-key lookup / lookupN
// calls (RingPop.lookup per request, index.js:434-451) through pinned, device-mapped host lines,
// so a call costs the PCIe round trips instead of a launch and a stream sync. Request: a header
// line {seq, len, np, W, stop} and up to kSvcChunks key lines of 60 B + their copy of seq in the
// last dword (the host writes a line's bytes before its seq, so a line read with the expected
// seq holds the new bytes). Response: owners + count, then seq in its own line, released at
// system scope. The wave exits on the stop flag, after idle_ticks of no request, or after
// max_ticks in all (s_memrealtime, 100 MHz), so it always drains; the host relaunches it when a
// request finds it gone.
constexpr uint32_t kSvcChunks = 3, kSvcKeyMax = kSvcChunks * 60;
constexpr uint32_t kSvcWaves = 8;     // k_lookup_service3's independent pollers (RP_SVC_WAVES)
constexpr uint32_t kSvcPeriod = 120;  // their common poll period, 100 MHz ticks (RP_SVC_PERIOD)
struct SvcLines {
    uint32_t req[16 * (1 + kSvcChunks)];  // header line + key lines
    uint32_t resp[16];                    // owners[0..W), count at [15]
    uint32_t resp_seq[16];                // [0] = the answered seq
    uint64_t resp2[8][8];                 // k_lookup_service3: slot seq % 8, owner q | seq << 32 (64-B lines)
    uint32_t diag[16];                    // k_lookup_service3 with prof: seq, then phase ticks (100 MHz)
};
// With the compact layout built, a key with 1..4 owners wanted takes compact_fix_walk (the
// index record, the bucket's tokens, the next 8 owners: three dependent trips) instead of the
// wide binary search and walk.
template <class View>
__global__ __launch_bounds__(64) void k_lookup_service(SvcLines* io, View rv, CompactFixView fv, uint32_t use_compact,
                                                       uint32_t last, uint64_t idle_ticks, uint64_t max_ticks) {
    __shared__ uint32_t kw[kSvcChunks * 15];
    const uint32_t lane = threadIdx.x;
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
    uint64_t t_idle = t_start;
    while (true) {
        const uint32_t v = lane < 16 * (1 + kSvcChunks)
                               ? __hip_atomic_load(&io->req[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                               : 0u;
        const uint32_t seq = __builtin_amdgcn_readfirstlane(__shfl(v, 0, 64));
        const uint32_t stop = __builtin_amdgcn_readfirstlane(__shfl(v, 4, 64));
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        if (stop || now - t_start > max_ticks) break;
        if (seq == last) {
            if (now - t_idle > idle_ticks) break;
            __builtin_amdgcn_s_sleep(2);
            continue;
        }
        const uint32_t len = __builtin_amdgcn_readfirstlane(__shfl(v, 1, 64));
        const int np = (int)__builtin_amdgcn_readfirstlane(__shfl(v, 2, 64));
        const uint32_t W = __builtin_amdgcn_readfirstlane(__shfl(v, 3, 64));
        const uint32_t nch = (len + 59) / 60;
        // every key line the request uses must carry this seq (else re-read)
        const bool line_ok = lane < 16 || (lane >> 4) > nch || (lane & 15) != 15 || v == seq;
        if (__ballot(!line_ok) != 0 || len > kSvcKeyMax || W > 16) {
            if (len > kSvcKeyMax || W > 16) {  // malformed: answer empty
                if (lane < 16) __hip_atomic_store(&io->resp[lane], lane == 15 ? 0u : NIL, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_SYSTEM);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
                if (lane == 0) __hip_atomic_store(&io->resp_seq[0], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                last = seq;
                t_idle = now;
            }
            continue;
        }
        if (lane >= 16 && (lane & 15) < 15) kw[((lane >> 4) - 1) * 15 + (lane & 15)] = v;
        __syncthreads();
        uint32_t res[8] = {NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL};
        int c = 0;
        if (lane == 0) {
            const uint32_t hk = fh::hash32(fh::PtrSrc{reinterpret_cast<const uint8_t*>(kw)}, len);
            if (use_compact && np >= 1 && np <= 4) {
                uint32_t r4[4];
                c = compact_fix_walk(fv, hk, np, r4);
#pragma unroll
                for (int q = 0; q < 4; q++) res[q] = r4[q];
            } else {
                c = ring_walk<8>(rv, rv.find(hk), np > 8 ? 8 : np, res);
            }
        }
        // lane 0's row to lanes 0..W-1, then the seq after it (system-scope release)
        uint32_t mine = NIL;
#pragma unroll
        for (uint32_t q = 0; q < 8; q++) {
            const uint32_t x = __shfl(res[q], 0, 64);
            mine = lane == q ? x : mine;
        }
        const uint32_t cnt = (uint32_t)__shfl(c, 0, 64);
        if (lane < 16) __hip_atomic_store(&io->resp[lane], lane == 15 ? cnt : (lane < W ? mine : NIL), __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_SYSTEM);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        if (lane == 0) __hip_atomic_store(&io->resp_seq[0], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        __syncthreads();
        last = seq;
        t_idle = __builtin_amdgcn_s_memrealtime();
    }
}

// One key on the compact layout in two dependent trips (the index record, one 5-entry window at
// the predicted start, as k_lookupn_lean): true with the first `need` distinct owners when window 1
// holds them; false when the key needs more (a fingerprint tie, a long bucket, the ring end, a
// position or repeated owners past the window), and the caller takes the exact walk.
__device__ __forceinline__ bool svc_compact_window(const CompactView& cv, uint32_t h, int need, uint32_t (&res)[4],
                                                   int& cnt) {
    const uint32_t bsh = 32u - cv.cb;
    const uint32_t g = h >> (bsh + 3u), s4 = ((h >> bsh) & 7u) * 4u;
    const u32x2 rec = *reinterpret_cast<const u32x2*>(cv.idx + 2ull * g);
    const uint32_t below = rec.y & ((1u << s4) - 1u);
    const uint32_t x = (below & 0x0F0F0F0Fu) + ((below >> 4) & 0x0F0F0F0Fu);
    const uint32_t lo = rec.x + ((x * 0x01010101u) >> 24);
    const uint32_t bc = (rec.y >> s4) & 15u;
    if (bc > 10u || lo + 20u > cv.M) return false;
    const uint32_t fl = (((h << cv.cb) >> 24) * bc) >> 8;
    const uint32_t w = (need >= 2 && fl > 1u) ? fl - 1u : 0u;
    const u32x4_a1 v = *reinterpret_cast<const u32x4_a1*>(cv.ent + 3ull * (lo + w));
    const uint32_t e[5] = {v.x & 0xFFFFFFu, (v.x >> 24) | ((v.y & 0xFFFFu) << 8), (v.y >> 16) | ((v.z & 0xFFu) << 16),
                           v.z >> 8, v.w & 0xFFFFFFu};
    const uint32_t omask = (1u << cv.ob) - 1u, obit = 1u << cv.ob;
    const uint32_t K = ((h & ((1u << bsh) - 1u)) >> cv.fsh) << cv.ob;
    uint32_t lt = 0;
    bool tie = false;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const bool inb = (uint32_t)j + w < bc;
        lt += (inb && e[j] < K);
        tie |= (inb && e[j] - K < obit);
    }
    if ((tie && !cv.exact) || (w > 0u && lt == 0u)) return false;
    const uint32_t rc = dedupe5(e, lt, omask, (uint32_t)need, res);
    if (rc < (uint32_t)need) return false;
    cnt = (int)rc;
    return true;
}

// The service's direct table (round 5): one 64-B record per bucket of the top B hash bits (2^B >= M,
// B >= 16, so the bucket fixes all but <= 16 token bits and a record answers exactly, no
// fingerprints), read as one aligned line: the lookup is one dependent trip instead of the compact
// layout's two. Record words:
//   [0]     token count c (<= 7; 15: more, the caller takes the other paths) | successors s << 8 |
//           complete << 16 (s < 16 only because the ring has fewer distinct owners)
//   [1..7]  the bucket's tokens in ring order: low 32 - B bits | owner << 16
//   [8..15] the first 16 distinct owners from the first token after the bucket onwards (cyclic),
//           two 16-bit ids a word
// lookupN(h, n <= 8) = the first n distinct of (owners of the bucket's tokens >= h, then the
// successors): the successors are the distinct owners of the rest of the walk in first-seen order,
// so deduplicating the concatenation gives the walk's answer (lib/ring/index.js:157-189). Only
// for rings whose interned ids fit 16 bits. tools/svc_latency.js prices it (r05w).
constexpr uint32_t kDtEnt = 7, kDtSucc = 16, kDtWalk = 4096;
__global__ __launch_bounds__(256) void k_dt_build(const uint32_t* __restrict__ tok, const uint32_t* __restrict__ own,
                                                  uint32_t M, uint32_t B, uint4* __restrict__ dt) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >> B) return;
    const uint32_t sh = 32u - B;
    auto lower = [&](uint64_t key) {  // first i with tok[i] >= key
        uint32_t lo = 0, hi = M;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((uint64_t)tok[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    const uint32_t lo = lower(b << sh), hi = lower((b + 1) << sh);
    const uint32_t c = hi - lo;
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = 0xFFFFFFFFu;
    if (c > kDtEnt) {
        w[0] = 15u;
    } else {
        for (uint32_t i = 0; i < c; i++) w[1 + i] = (tok[lo + i] & ((1u << sh) - 1u)) | (own[lo + i] << 16);
        uint32_t su[kDtSucc], ns = 0, k = 0;
        const uint32_t lim = M < kDtWalk ? M : kDtWalk;
        for (; k < lim && ns < kDtSucc; k++) {
            const uint32_t j = hi + k >= M ? hi + k - M : hi + k;
            const uint32_t o = own[j];
            bool seen = false;
            for (uint32_t q = 0; q < ns; q++) seen |= su[q] == o;
            if (!seen) su[ns++] = o;
        }
        const uint32_t complete = (ns < kDtSucc && k == M) ? 1u : 0u;
        w[0] = c | (ns << 8) | (complete << 16);
        for (uint32_t q = 0; q < kDtSucc; q += 2)
            w[8 + q / 2] = (q < ns ? su[q] : 0xFFFFu) | ((q + 1 < ns ? su[q + 1] : 0xFFFFu) << 16);
    }
    uint4* d = dt + 4 * b;
#pragma unroll
    for (int q = 0; q < 4; q++) d[q] = uint4{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
}

// The answer from a record, across the wave: lane i < 16 holds record word i (x). Lane i takes
// item i of (owners of the bucket's tokens >= h, then the successors), flags it when no earlier
// item has its owner, and the flagged items' ranks are their slots. Returns false (wave-uniform)
// when the record cannot say (an overflowing bucket, too few successors); else cnt and, in lane
// q < 8, the q-th owner (NIL past cnt).
__device__ __forceinline__ bool dt_answer(uint32_t x, uint32_t lane, uint32_t h, uint32_t B, uint32_t need,
                                          uint32_t* slot, uint32_t& mine, int& cnt) {
    const uint32_t w0 = __builtin_amdgcn_readfirstlane(x);
    const uint32_t c = w0 & 15u, ns = (w0 >> 8) & 31u, complete = (w0 >> 16) & 1u;
    if (c > kDtEnt) return false;
    const uint32_t rmask = (1u << (32u - B)) - 1u, hr = h & rmask;
    const uint32_t e = __shfl(x, 1 + (lane < kDtEnt ? lane : 0), 64);
    const uint32_t f = (uint32_t)__popcll(__ballot(lane < c && (e & 0xFFFFu & rmask) < hr));  // tokens below h
    const uint32_t na = c - f;
    const uint32_t ea = __shfl(x, 1 + f + (lane < na ? lane : 0), 64);
    const uint32_t k = lane - na;
    const uint32_t sw = __shfl(x, 8 + ((lane >= na && k < kDtSucc ? k : 0) >> 1), 64);
    const bool valid = lane < na || (lane >= na && k < ns);
    const uint32_t t = lane < na ? (ea >> 16) : ((sw >> (16 * (k & 1))) & 0xFFFFu);
    bool dup = false;
#pragma unroll
    for (uint32_t j = 0; j < kDtEnt + kDtSucc; j++) {
        const uint32_t tj = __builtin_amdgcn_readlane(t, j);
        dup |= j < lane && tj == t;
    }
    const uint64_t fb = __ballot(valid && !dup);
    const uint32_t total = (uint32_t)__popcll(fb);
    if (total < need && !complete) return false;
    const uint32_t rank = (uint32_t)__popcll(fb & ((1ull << lane) - 1ull));
    if (valid && !dup && rank < 8) slot[rank] = t;
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the slots are written (one wave: no barrier)
    __builtin_amdgcn_wave_barrier();
    const uint32_t got = total < need ? total : need;
    mine = lane < got ? slot[lane] : NIL;
    cnt = (int)got;
    return true;
}

// dt_answer without LDS (round 6, the default; RP_SVC_ANS=0 keeps dt_answer): the items stay where
// the record puts them, in item order by lane (the bucket's tokens >= h in lanes 1..c, the
// successors spread to lanes 16..31 by one shuffle), and the first `need` distinct owners are
// taken one at a time: the first remaining lane's owner, then every lane holding it dropped by a
// ballot. A lookup (need 1) is one step; no 23-step duplicate scan, no LDS slots.
__device__ __forceinline__ bool dt_answer_fast(uint32_t x, uint32_t lane, uint32_t h, uint32_t B, uint32_t need,
                                               uint32_t& mine, int& cnt) {
    const uint32_t w0 = __builtin_amdgcn_readlane(x, 0);
    const uint32_t c = w0 & 15u, ns = (w0 >> 8) & 31u, complete = (w0 >> 16) & 1u;
    if (c > kDtEnt) return false;
    const uint32_t rmask = (1u << (32u - B)) - 1u, hr = h & rmask;
    const uint32_t k = lane - 16u;
    const bool sl = lane >= 16u && k < kDtSucc;
    const uint32_t sw = __shfl(x, 8u + ((sl ? k : 0u) >> 1), 64);
    const bool tk = lane >= 1u && lane <= c && (x & 0xFFFFu & rmask) >= hr;
    const bool su = sl && k < ns;
    const uint32_t t = tk ? (x >> 16) : ((sw >> (16u * (k & 1u))) & 0xFFFFu);
    uint64_t rem = __ballot(tk || su);
    uint32_t got = 0;
    mine = NIL;
    while (got < need && rem) {
        const uint32_t v = __builtin_amdgcn_readlane(t, (uint32_t)__builtin_ctzll(rem));
        mine = lane == got ? v : mine;
        rem &= ~__ballot(t == v);
        got++;
    }
    if (got < need && !complete) return false;
    cnt = (int)got;
    return true;
}

// The lookup service, round 5 form (RP_RING_SVC=2, the default). Round 5 measured the round-4
// kernel's call (5.0 us in node) with device stamps (RP_SVC_PROF): the poll's PCIe round trip
// ~1.1 us, the key's farmhash on one lane from LDS ~0.5 us, three dependent table trips, the
// answer's line and its seq line. A three-wave form (a poller with 8 reads in flight, a worker,
// an L2-warming wave) was slower (6.0 us): the poller's PCIe reads in flight delayed the worker's
// table loads on the same CU (lookup 1.4 us at 1 read in flight, 2.8 at 8) and the LDS hand-off
// cost 0.4 us. So this form is one wave again, and:
//   - the host hashes the key (farmhash32, as the reference's lookup does on the CPU) and sends
//     {seq, hash, np, W, stop, ..., seq} in one 64-B header line: no key lines, no device hash,
//     and no key-length limit;
//   - one poll in flight, and nothing else outstanding when a request is seen;
//   - the compact layout answers in two trips (svc_compact_window: the index record and one
//     window), the exact walk otherwise;
//   - the answer is one 64-B line of 8 words {owner | seq << 32} (no fence, no second line: the
//     host takes the line when every word carries its seq);
//   - RP_SVC_WARM=1: while idle, after each poll is issued, the wave touches 32 KB of the compact
//     tables (the whole 3.5 MB about every 0.15 ms) to keep them in its XCD's L2. Measured without
//     effect on the lookup's two trips (1.08 us either way, r05g) and 0.1 us slower polls: off.
// Round 6: the wait for a request is the poll's phase, on average half a PCIe round trip before
// the read that sees the line plus the return. So the service is kSvcWaves independent waves of
// this same loop, one workgroup each (so on different CUs and XCDs, none delaying another's table
// read), each with its one poll in flight at its own phase: the first to see a request answers
// it, the later ones answer it again with the same line (a pure function of the request), and no
// wave waits on another. The answer goes to line seq % 8, so a late duplicate can only land on
// the line of a request eight calls old, never on the one the host is waiting for.
// RP_SVC_PROF=1 writes per-call device phase ticks into diag (poll round trip, lookup).
template <class View>
__global__ __launch_bounds__(64) void k_lookup_service3(SvcLines* io, View rv, CompactFixView fv, CompactView cv,
                                                       uint32_t use_compact, uint32_t last, uint64_t idle_ticks,
                                                       uint64_t max_ticks, uint32_t warm, uint32_t prof,
                                                       const uint32_t* __restrict__ dt, uint32_t dtb,
                                                       uint32_t period, uint32_t ans_old) {
    __shared__ uint32_t dslot[8];
    const uint32_t lane = threadIdx.x;
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
    uint64_t t_idle = t_start;
    const uint64_t nidx = cv.idx_bytes, nwarm = nidx + cv.ent_bytes;
    uint64_t woff = 0;
    uint32_t acc = 0;
    // period > 0 (several waves): wave i issues its polls on the device clock's slots
    // n * period + i * period / waves, so the waves' reads reach the host line evenly spread
    // instead of in step (launched together, they would otherwise poll at one phase)
    uint64_t slot = period ? (t_start / period + 1) * period + (uint64_t)blockIdx.x * period / gridDim.x : 0;
    while (true) {
        if (period) {
            while (__builtin_amdgcn_s_memrealtime() < slot) __builtin_amdgcn_s_sleep(1);
            const uint64_t t = __builtin_amdgcn_s_memrealtime();
            do slot += period;
            while (slot <= t);
        }
        if (warm == 2 && dt) {  // this wave's slice of the direct table, a record a lane per poll, issued
            // before the poll (loads return in order: one behind the poll would hold up the lookup's)
            const uint64_t nrec = 1ull << dtb, r0 = nrec * blockIdx.x / gridDim.x, r1 = nrec * (blockIdx.x + 1) / gridDim.x;
            const uint64_t r = r0 + woff + lane;
            acc ^= r < r1 ? dt[16ull * r] : 0u;
            woff = r0 + woff + 64 >= r1 ? 0 : woff + 64;
        }
        const uint64_t tp = __builtin_amdgcn_s_memrealtime();
        const uint32_t v = lane < 16 ? __hip_atomic_load(&io->req[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
        if (warm == 1 && use_compact) {  // issued after the poll, done within its round trip
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint64_t o = woff + 64ull * lane;
                const uint32_t x = o < nidx ? cv.idx[o >> 2]
                                   : o + 4 <= nwarm ? *reinterpret_cast<const uint32_t*>(cv.ent + ((o - nidx) & ~3ull))
                                                    : 0u;
                acc ^= x;
                woff = woff + 4096 >= nwarm ? 0 : woff + 4096;
            }
        }
        const uint32_t seq = __builtin_amdgcn_readlane(v, 0);  // (register reads, no LDS trip)
        const uint32_t stop = __builtin_amdgcn_readlane(v, 4);
        const uint32_t tail = __builtin_amdgcn_readlane(v, 15);
        if (prof) asm volatile("s_waitcnt vmcnt(0)" ::"s"(seq) : "memory");  // (stamps) the clock after the poll
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        if (stop || now - t_start > max_ticks) break;
        if (seq == last || tail != seq) {
            if (seq == last && now - t_idle > idle_ticks) break;
            __builtin_amdgcn_s_sleep(2);
            continue;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the warm load, before the lookup's own
        asm volatile("" ::"v"(acc));
        const uint32_t hk = __builtin_amdgcn_readlane(v, 1);
        const int np = (int)__builtin_amdgcn_readlane(v, 2);
        const uint32_t W = __builtin_amdgcn_readlane(v, 3);
        uint32_t res[8] = {NIL, NIL, NIL, NIL, NIL, NIL, NIL, NIL};
        uint32_t path = 0;
        bool dok = false;
        uint32_t dmine = NIL;
        if (dt && np >= 1 && np <= 8) {  // the direct table: one 64-B line, lanes 0..15
            const uint32_t x = lane < 16 ? dt[16ull * (hk >> (32u - dtb)) + lane] : 0u;
            int c = 0;
            dok = ans_old ? dt_answer(x, lane, hk, dtb, (uint32_t)np, dslot, dmine, c)
                          : dt_answer_fast(x, lane, hk, dtb, (uint32_t)np, dmine, c);
            path = dok ? 4u : 0u;
        }
        uint32_t o = dmine;
        if (!dok) {  // (wave-uniform) the compact window or the walks, on lane 0
            if (lane == 0) {
                bool ok = false;
                if (use_compact && np >= 1 && np <= 4) {
                    uint32_t r4[4] = {NIL, NIL, NIL, NIL};
                    int c = 0;
                    ok = svc_compact_window(cv, hk, np, r4, c);
                    path = ok ? 1u : 2u;
                    if (!ok) {
                        c = compact_fix_walk(fv, hk, np, r4);
                        ok = true;
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) res[q] = r4[q];
                }
                if (!ok) {
                    ring_walk<8>(rv, rv.find(hk), np > 8 ? 8 : np, res);
                    path = 3;
                }
            }
#pragma unroll
            for (uint32_t q = 0; q < 8; q++) {
                const uint32_t x = __shfl(res[q], 0, 64);
                o = lane == q ? x : o;
            }
        }
        if (prof) {  // diag: seq, poll round trip, lookup (ticks), path
            asm volatile("" ::"v"(o));
            const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
            const uint32_t pth = (uint32_t)__shfl(path, 0, 64);
            const uint32_t d[4] = {seq, (uint32_t)(now - tp), (uint32_t)(t1 - now), pth};
            uint32_t dv = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) dv = lane == (uint32_t)q ? d[q] : dv;
            if (lane < 4) __hip_atomic_store(&io->diag[lane], dv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (lane < 8)
            __hip_atomic_store(&io->resp2[seq & 7u][lane], (uint64_t)(lane < W ? o : NIL) | ((uint64_t)seq << 32),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        last = seq;
        t_idle = __builtin_amdgcn_s_memrealtime();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" ::"v"(acc));
}

// ---- build kernels ----

// tokens[a*R + i] = farmhash32(name(ids[a]) + String(i)); owners likewise = ids[a].
__global__ void k_replica_tokens(const uint8_t* __restrict__ names, const uint64_t* __restrict__ noff,
                                 const uint32_t* __restrict__ ids, uint32_t n_srv, uint32_t R,
                                 uint32_t* __restrict__ tok, uint32_t* __restrict__ own) {
    const uint64_t total = (uint64_t)n_srv * R;
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += gstride) {
        const uint32_t a = (uint32_t)(k / R), i = (uint32_t)(k % R);
        const uint32_t id = ids[a];
        fh::ReplicaSrc s;
        s.name = names + noff[id];
        s.nlen = (uint32_t)(noff[id + 1] - noff[id]);
        const uint32_t nd = fh::decimal(i, s.dig);
        tok[k] = fh::hash32(s, s.nlen + nd);
        own[k] = id;
    }
}

// owners for caller-supplied tokens
__global__ void k_expand_owner(const uint32_t* __restrict__ ids, uint32_t n_srv, uint32_t R,
                               uint32_t* __restrict__ own) {
    const uint64_t total = (uint64_t)n_srv * R;
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += gstride)
        own[k] = ids[k / R];
}

__device__ __forceinline__ uint32_t lower_bound_dev(const uint32_t* a, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// keep sorted-new token p iff first of its equal run (stable sort => first inserted) and
// absent from the live ring (insert-if-absent, rbtree.js:112-116).
__global__ void k_mark_new(const uint32_t* __restrict__ ntok, uint32_t K, const uint32_t* __restrict__ tok,
                           uint32_t M, uint32_t* __restrict__ flag) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < K; p += gstride) {
        const uint32_t t = ntok[p];
        bool keep = (p == 0) || (ntok[p - 1] != t);
        if (keep && M) {
            const uint32_t i = lower_bound_dev(tok, M, t);
            keep = !(i < M && tok[i] == t);
        }
        flag[p] = keep ? 1u : 0u;
    }
}

__global__ void k_compact_pairs(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin,
                                const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                uint32_t n, uint32_t* __restrict__ kout, uint32_t* __restrict__ vout) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gstride)
        if (flag[p]) {
            kout[pos[p]] = kin[p];
            vout[pos[p]] = vin[p];
        }
}

// Merge two sorted, mutually disjoint token arrays (rank = own index + rank in the other).
__global__ void k_merge(const uint32_t* __restrict__ at, const uint32_t* __restrict__ ao, uint32_t na,
                        const uint32_t* __restrict__ bt, const uint32_t* __restrict__ bo, uint32_t nb,
                        uint32_t* __restrict__ ot, uint32_t* __restrict__ oo) {
    const uint64_t total = (uint64_t)na + nb;
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gstride) {
        if (p < na) {
            const uint32_t t = at[p];
            const uint32_t d = (uint32_t)p + lower_bound_dev(bt, nb, t);
            ot[d] = t;
            oo[d] = ao[p];
        } else {
            const uint32_t q = (uint32_t)(p - na);
            const uint32_t t = bt[q];
            const uint32_t d = q + lower_bound_dev(at, na, t);
            ot[d] = t;
            oo[d] = bo[q];
        }
    }
}

// erase-by-key (rbtree.js:152-232): mark every live token equal to a removal token.
__global__ void k_mark_del(const uint32_t* __restrict__ rtok, uint64_t K, const uint32_t* __restrict__ tok,
                           uint32_t M, uint32_t* __restrict__ keep) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < K; p += gstride) {
        const uint32_t t = rtok[p];
        const uint32_t i = lower_bound_dev(tok, M, t);
        if (i < M && tok[i] == t) keep[i] = 0u;
    }
}

__global__ void k_fill_u32(uint32_t* p, uint64_t n, uint32_t v) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gstride) p[i] = v;
}

__global__ void k_bucket_index(const uint32_t* __restrict__ tok, uint32_t M, uint32_t bbits,
                               uint32_t* __restrict__ bstart) {
    const uint64_t nbk = (1ull << bbits);
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b <= nbk; b += gstride) {
        if (b == nbk) bstart[b] = M;
        else bstart[b] = lower_bound_dev(tok, M, (uint32_t)(b << (32 - bbits)));
    }
}

__global__ void k_pack(const uint32_t* __restrict__ tok, const uint32_t* __restrict__ own, uint32_t M,
                       uint32_t B, uint32_t* __restrict__ ent) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < (uint64_t)M + kEntPad; j += gstride)
        ent[j] = j < M ? ((tok[j] << B) | own[j]) : 0xFFFFFFFFu;
}

// compact entries: 3 bytes per token, (fp << ob) | owner; padding entries are all ones
__global__ void k_pack3(const uint32_t* __restrict__ tok, const uint32_t* __restrict__ own, uint32_t M,
                        uint32_t cb, uint32_t ob, uint32_t fsh, uint8_t* __restrict__ ent) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t rmask = cb == 0 ? 0xFFFFFFFFu : ((1u << (32u - cb)) - 1u);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < (uint64_t)M + kEnt3Pad + 6; j += gstride) {
        const uint32_t v = j < M ? ((((tok[j] & rmask) >> fsh) << ob) | own[j]) : 0xFFFFFFu;
        ent[3 * j + 0] = (uint8_t)v;
        ent[3 * j + 1] = (uint8_t)(v >> 8);
        ent[3 * j + 2] = (uint8_t)(v >> 16);
    }
}

// compact index: per group of 8 buckets {first position, 8 x 4-bit counts}; *over is set when a
// bucket holds more than 15 tokens (the layout is then not used)
__global__ void k_cindex(const uint32_t* __restrict__ bst, uint32_t ngroups, uint32_t* __restrict__ idx,
                         uint32_t* __restrict__ over) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += gstride) {
        uint32_t nib = 0;
        bool bad = false;
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const uint32_t c = bst[g * 8 + s + 1] - bst[g * 8 + s];
            bad |= c > 15u;
            nib |= (c > 15u ? 15u : c) << (4 * s);
        }
        idx[2 * g] = bst[g * 8];
        idx[2 * g + 1] = nib;
        if (bad) atomicOr(over, 1u);
    }
}

// The hinted index of the lean kernel's lookupN(3) (round 5): per group g of 8 buckets,
// x = (base - pred(g)) & 0x3FFF | hints << 14 and y = the nibble counts (as k_cindex), pred(g) =
// g * M >> (cb - 3). Bucket s's 2-bit hint h moves window 1's start to max(0, fl - 1 + h - 1)
// (fl = the key's 8 top residual bits x count >> 8, the lean kernel's prediction): of the three,
// the start whose window resolves the largest share of the bucket's hash range (a key whose
// position in the bucket is rel resolves at w = 0 when rel <= 2, at w > 0 when rel is w + 1 or
// w + 2). Buckets of more than 10 tokens keep w = 0 (hint 1). over |= 1 when a base delta does
// not fit 14 bits (the lean kernel then runs without hints).
__global__ void k_cindex_hint(const uint32_t* __restrict__ tok, const uint32_t* __restrict__ bst, uint32_t M,
                              uint32_t cb, uint32_t ngroups, uint32_t* __restrict__ idx, uint32_t* __restrict__ over) {
    const uint32_t bsh = 32u - cb;
    const uint32_t qsh = bsh - 8u;  // residual >> qsh = the 8 bits the kernel's prediction reads
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += gstride) {
        const uint32_t base = bst[g * 8];
        const int64_t delta = (int64_t)base - (int64_t)(((uint64_t)g * M) >> (cb - 3));
        if (delta < -8192 || delta > 8191) atomicOr(over, 1u);
        uint32_t nib = 0, hints = 0;
        for (int s = 0; s < 8; s++) {
            const uint32_t lo = bst[g * 8 + s], bc = bst[g * 8 + s + 1] - lo;
            nib |= (bc > 15u ? 15u : bc) << (4 * s);
            uint32_t best = 1;
            if (bc <= 10u) {
                // resolved length of the hash range for each hint, walking the 256 prediction
                // slices and the bucket's token residuals in order
                uint64_t g0 = 0, g1 = 0, g2 = 0;  // resolved lengths for hints 0, 1, 2
                uint32_t j = 0;  // tokens below the slice start
                const uint64_t S = 1ull << qsh;
                for (uint32_t q = 0; q < 256; q++) {
                    const uint32_t fl = (q * bc) >> 8;
                    uint64_t a = (uint64_t)q * S;
                    const uint64_t e = a + S;
                    uint32_t rel = j;
                    while (true) {
                        // [a, nxt) has position rel
                        const uint64_t tn = rel < bc ? (uint64_t)(tok[lo + rel] & ((1u << bsh) - 1u)) + 1ull : e;
                        const uint64_t nxt = tn < e ? tn : e;
                        if (nxt > a) {
                            auto ok = [&](int w0) {
                                const uint32_t w = w0 > 0 ? (uint32_t)w0 : 0u;
                                return w == 0 ? rel <= 2u : (rel == w + 1 || rel == w + 2);
                            };
                            g0 += ok((int)fl - 2) ? nxt - a : 0;
                            g1 += ok((int)fl - 1) ? nxt - a : 0;
                            g2 += ok((int)fl) ? nxt - a : 0;
                            a = nxt;
                        }
                        if (a >= e) break;
                        rel++;
                    }
                    while (j < bc && (uint64_t)(tok[lo + j] & ((1u << bsh) - 1u)) < e) j++;
                }
                best = (g1 >= g0 && g1 >= g2) ? 1u : (g0 >= g2 ? 0u : 2u);
            }
            hints |= best << (2 * s);
        }
        idx[2 * g] = ((uint32_t)delta & 0x3FFFu) | (hints << 14);
        idx[2 * g + 1] = nib;
    }
}

// The LDS-index layout (round 6; k_lookupn_lds). The bucket search structure moves out of L2 into
// every CU's LDS, so a key takes one L2 trip (its window) instead of two (index record, then
// window). NG groups (a power of two, <= 8,192: 128 KB) of 28 buckets, NB = 28 NG buckets over the
// hash space: a hash h is in group g = h >> (32 - lg) and bucket j = floor(28 x / 2^32) of it, with
// x = h << lg, and its fingerprint is the top fb bits of the remainder (28 x) mod 2^32 (monotone in
// h within a bucket). A group record is 16 B: 28 4-bit token counts, then the group's first
// position as an int16 delta from pred(g) = g M / NG. Entries are 3 B, (fp << ob) | owner.
__device__ __forceinline__ uint32_t lds_first_pos(const uint32_t* __restrict__ tok, uint32_t M, uint32_t lg,
                                                  uint32_t g, uint32_t j) {
    // the least h in bucket (g, j): x >= ceil(j 2^32 / 28)
    const uint64_t xm = ((uint64_t)j << 32) / 28u + (((uint64_t)j << 32) % 28u ? 1u : 0u);
    const uint64_t hm = ((uint64_t)g << (32 - lg)) + (xm >> lg) + ((xm & ((1ull << lg) - 1u)) ? 1u : 0u);
    return hm >= (1ull << 32) ? M : lower_bound_dev(tok, M, (uint32_t)hm);
}
__global__ void k_lidx_build(const uint32_t* __restrict__ tok, uint32_t M, uint32_t lg, uint32_t ng,
                             uint4* __restrict__ idx, uint32_t* __restrict__ over) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += gstride) {
        uint32_t w[4] = {0, 0, 0, 0};
        uint32_t p = lds_first_pos(tok, M, lg, (uint32_t)g, 0);
        const uint32_t base = p;
        bool full = false;
        for (uint32_t j = 0; j < 28; j++) {
            const uint32_t q = j == 27 ? (g + 1 == ng ? M : lds_first_pos(tok, M, lg, (uint32_t)g + 1, 0))
                                       : lds_first_pos(tok, M, lg, (uint32_t)g, j + 1);
            const uint32_t c = q - p;
            full |= c > 15u;
            w[j >> 3] |= (c > 15u ? 15u : c) << (4 * (j & 7));
            p = q;
        }
        const int64_t delta = (int64_t)base - (int64_t)(((uint64_t)g * M) >> lg);
        if (delta < -32767 || delta > 32767) atomicOr(over, 1u);
        // a bucket of 16+ tokens: the counts no longer sum to positions, so every key of the group
        // takes the exact path (delta -32768 marks it)
        w[3] |= (full ? 0x8000u : ((uint32_t)delta & 0xFFFFu)) << 16;
        idx[g] = uint4{w[0], w[1], w[2], w[3]};
    }
}
// LDS-index entries: 3 bytes per token, (fp << ob) | owner; padding entries are all ones
__global__ void k_lpack3(const uint32_t* __restrict__ tok, const uint32_t* __restrict__ own, uint32_t M, uint32_t lg,
                         uint32_t fb, uint32_t ob, uint8_t* __restrict__ ent) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < (uint64_t)M + kEnt3Pad + 6; j += gstride) {
        uint32_t v = 0xFFFFFFu;
        if (j < M) {
            const uint32_t x = tok[j] << lg;
            const uint32_t fp = (uint32_t)((uint64_t)x * 28u) >> (32u - fb);
            v = (fp << ob) | own[j];
        }
        ent[3 * j + 0] = (uint8_t)v;
        ent[3 * j + 1] = (uint8_t)(v >> 8);
        ent[3 * j + 2] = (uint8_t)(v >> 16);
    }
}

// checksum string pieces: len of (name + ';') for in-ring servers in name order.
__global__ void k_ck_len(const uint32_t* __restrict__ sorted_ids, uint32_t n,
                         const uint8_t* __restrict__ in_ring, const uint64_t* __restrict__ noff,
                         uint32_t* __restrict__ len) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gstride) {
        const uint32_t id = sorted_ids[i];
        len[i] = in_ring[id] ? (uint32_t)(noff[id + 1] - noff[id]) + 1u : 0u;
    }
}

__global__ void k_ck_scatter(const uint32_t* __restrict__ sorted_ids, uint32_t n,
                             const uint8_t* __restrict__ in_ring, const uint8_t* __restrict__ names,
                             const uint64_t* __restrict__ noff, const uint32_t* __restrict__ pos,
                             uint8_t* __restrict__ buf) {
    // one wave per name: lanes copy bytes
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = wid; i < n; i += nw) {
        const uint32_t id = sorted_ids[i];
        if (!in_ring[id]) continue;
        const uint64_t b = noff[id];
        const uint32_t L = (uint32_t)(noff[id + 1] - b);
        const uint32_t p = pos[i];
        for (uint32_t q = lane; q < L; q += 64) buf[p + q] = names[b + q];
        if (lane == 0) buf[p + L] = ';';
    }
}

__global__ void k_hash_batch(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n,
                             uint32_t* __restrict__ out) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gstride)
        out[k] = fh::hash32(fh::PtrSrc{bytes + off[k]}, (uint32_t)(off[k + 1] - off[k]));
}

__global__ void k_gen_uuid(uint32_t seed, uint64_t k0, uint64_t n, uint32_t* __restrict__ out) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gstride) {
        uint32_t w[9];
        uuid_key_words(seed, k0 + k, w);
#pragma unroll
        for (int j = 0; j < 9; j++) out[k * 9 + j] = w[j];
    }
}

}  // namespace

// ---------------------------------------------------------------------------------- handle

// The scratch of the owner-load calls of one handle (a ring or a snapshot), ordered across
// streams as Scratch is: a call on another stream first waits for the previous call's work.
struct LoadScratch {
    DevBuf<uint32_t> rows;             // one chunk's rows
    DevBuf<unsigned long long> out;    // the host forms' counters and the shares
    StreamOrder order;
    void use_on(hipStream_t st) { order.use_on(st); }
};

// The scratch of the moved-ranges calls of one handle (the ring now, or the `after` snapshot),
// ordered across streams in the same way.
struct RangeScratch {
    DevBuf<uint32_t> val, mi, mj;  // the merged tokens and their first-token positions in both rings
    DevBuf<uint32_t> tot;          // heads per tile, then their exclusive scan
    DevBuf<uint8_t> flg;           // per merged element: kRngHead | kRngTailPrev | kRngFinal
    DevBuf<uint32_t> io;           // the host forms' outputs
    StreamOrder order;
    void use_on(hipStream_t st) { order.use_on(st); }
};

// The scratch of the hand-off calls of one ring, ordered across streams in the same way.
struct HandoffScratch {
    DevBuf<uint32_t> key, dst, src, perm;  // the record stream's columns, and the sort's values
    DevBuf<uint8_t> slot;
    DevBuf<uint32_t> rank;  // per server id: 1 if a destination, then the exclusive scan (its group)
    DevBuf<uint32_t> io;    // the host forms' outputs
    StreamOrder order;
    void use_on(hipStream_t st) { order.use_on(st); }
};

// The scratch of the routing-agreement calls of one ring, ordered across streams in the same way.
struct RouteScratch {
    DevBuf<unsigned long long> plane;  // [id bound][view words]: the views that allow each server
    DevBuf<unsigned long long> meta;   // any[view words] | active[view words] | truth allows anybody
    DevBuf<uint8_t> tr;                // per server id: allowed by the truth
    DevBuf<unsigned long long> scan;   // route_share: aggregates [chunks][4][view words] | carries [chunks][2][view words]
    DevBuf<uint8_t> io8;               // the host form's rows, truth and active bytes
    DevBuf<uint32_t> io32;             // the host form's column map and uint32 outputs
    DevBuf<unsigned long long> io64;   // the host form's wrong | lost
    StreamOrder order;
    void use_on(hipStream_t st) { order.use_on(st); }
};

// Every environment variable of the batch-lookup launch path (A/B and diagnostics; none is API).
// lookup_knobs() reads them at every call and nothing keeps them: the tests and tools/ab_*.py
// change them between calls of one process. Which kernel a value selects: launch_lookupn below.
struct LookupKnobs {
    // RP_RING_WIDE: neither the compact nor the packed layout, the wide binary-search kernels
    bool wide;
    // RP_RING_LAYOUT=packed: not the compact layout, the packed probe kernel
    bool layout_packed;
    // RP_RING_NOWINDOW: the packed layout through the generic kernels, not the window probe
    bool nowindow;
    // RP_LOOKUP_ABLATE: timing ablations (results wrong) of the fixed, probe and compact kernels
    bool ablate_set;  // set at all, "0" too: the LDS-index kernel stays off (tools/ab_cb.py)
    int ablate;       // its number: CompactView::ablate, the fixed and probe kernels' MODE
    // RP_LOOKUP_WPRED=0: window 1 at the bucket start, not the predicted start
    bool wpred;
    // RP_LOOKUP_HINT=0: lookupN(3) without the hinted index
    bool hint;
    // RP_LOOKUP_LDS=1: the LDS-index kernel; any other value keeps it off (unset: kLdsDefault)
    bool lds;
    // RP_LOOKUP_LDS_GRID: its workgroups (0: unset, one a CU)
    uint64_t lds_grid;
    // RP_LOOKUP_LDS_STG=1: its keys through coalesced loads transposed in LDS
    bool lds_stg;
    // RP_LOOKUP_LDS_ABL: its timing ablations for lookupN(3) (results wrong)
    int lds_abl;
    // RP_LOOKUP_WS="NP:NC": the wave-specialised kernel with NP producer and NC consumer waves
    bool ws;             // set and not "0"
    int ws_np, ws_nc;    // "1" or any text without ':' means 1:3; a malformed pair gives ws_np = 0
    // RP_LOOKUP_WS_GRID: its workgroups (0: unset, what fits the CUs)
    uint64_t ws_grid;
    // RP_LOOKUP_WS_ABL: timing ablations of its 4:12 shape (results wrong)
    int ws_abl;
    // RP_LOOKUP_KPL: keys per lane of the compact, lean and probe kernels
    bool kpl_set;  // set, whatever the value: no sorted and no wave-specialised kernel
    int kpl;       // its number; each path maps it to the tiles it has
    // RP_LOOKUP_SORT: threads of the sorted-tile kernel, 0 = off (unset: kSortDefault)
    int sort_t;
    // RP_LOOKUP_GRID: workgroups of the sorted, lean and compact kernels (0: unset); the sorted
    // kernel it names is the strided one
    uint64_t grid;
    // RP_LOOKUP_TICKET: the 256-thread sorted tiles by ticket on a resident grid (1) or strided
    // over RP_LOOKUP_GRID's default (0); -1: unset (kTicketDefault)
    int ticket;
    // RP_LOOKUP_STAGGER: the ticketed form's start stagger, sixteenths of a tile time between the
    // resident workgroups of a CU (0: off; -1: unset, kStaggerDefault)
    int stagger;
    // RP_LOOKUP_TICKET_GRID: the ticketed form's workgroups, not capped at the tile count (tests
    // only; 0: unset, what is resident)
    uint64_t ticket_grid;
    // RP_LK_TL_DUMP: the file a -DRP_LK_TL (or -DRP_LK_PROF) build writes the sorted launch's timeline to
    const char* tl_dump;
    // RP_LOOKUP_LEAN=0: the round-1 compact kernel, not the lean one
    bool lean_set;  // set, whatever the value: no sorted kernel
    bool lean;
    // RP_LOOKUP_HALF: LDS slices of the lean kernel's key stage (2, 4)
    bool half_set;  // set, whatever the value: no sorted kernel
    int half;
    // RP_LOOKUP_FUSEFIX: deferred keys finished by the lean kernel's own workgroups; no sorted kernel
    bool fusefix;
    // RP_LOOKUP_STG: the lean kernel's key slices by DMA (1: compiler-issued, 2: from asm)
    bool stg_set;  // set, whatever the value: no sorted kernel
    int stg;
    // RP_LOOKUP_LH: the lean kernel's lookups in 1 or 2 halves (0: unset or not positive)
    bool lh_set;  // set, whatever the value: no sorted kernel
    uint64_t lh;
    // RP_LOOKUP_STGHS: key slices of RP_LOOKUP_STG=2 (4, 8)
    uint64_t stghs;
    // RP_LOOKUP_DEBUG: a census of the deferred keys on stderr after every tiled launch
    bool debug;
    // RP_LK_PROF_PRINT: the phase cycle counters of a -DRP_LK_PROF build on stderr
    bool prof_print;
};
static LookupKnobs lookup_knobs() {
    const auto num = [](const char* v) { return v ? atoi(v) : 0; };
    const auto is0 = [](const char* v) { return v && !strcmp(v, "0"); };
    const char *lay = getenv("RP_RING_LAYOUT"), *abl = getenv("RP_LOOKUP_ABLATE"), *lds = getenv("RP_LOOKUP_LDS"),
               *ws = getenv("RP_LOOKUP_WS"), *kpl = getenv("RP_LOOKUP_KPL"), *sort = getenv("RP_LOOKUP_SORT"),
               *lean = getenv("RP_LOOKUP_LEAN"), *half = getenv("RP_LOOKUP_HALF"), *stg = getenv("RP_LOOKUP_STG"),
               *tick = getenv("RP_LOOKUP_TICKET"), *stag = getenv("RP_LOOKUP_STAGGER");
    LookupKnobs k;
    k.wide = getenv_flag("RP_RING_WIDE");
    k.layout_packed = lay && !strcmp(lay, "packed");
    k.nowindow = getenv_flag("RP_RING_NOWINDOW");
    k.ablate_set = abl != nullptr;
    k.ablate = num(abl);
    k.wpred = !is0(getenv("RP_LOOKUP_WPRED"));
    k.hint = !is0(getenv("RP_LOOKUP_HINT"));
    k.lds = lds ? !strcmp(lds, "1") : kLdsDefault;
    k.lds_grid = env_pos("RP_LOOKUP_LDS_GRID", 0);
    k.lds_stg = (int)env_pos("RP_LOOKUP_LDS_STG", 0) == 1;
    k.lds_abl = num(getenv("RP_LOOKUP_LDS_ABL"));
    k.ws = ws && !is0(ws);
    k.ws_np = 1, k.ws_nc = 3;
    if (k.ws && strchr(ws, ':') && sscanf(ws, "%d:%d", &k.ws_np, &k.ws_nc) != 2) k.ws_np = 0;
    k.ws_grid = env_pos("RP_LOOKUP_WS_GRID", 0);
    k.ws_abl = num(getenv("RP_LOOKUP_WS_ABL"));
    k.kpl_set = kpl != nullptr;
    k.kpl = num(kpl);
    k.sort_t = sort ? atoi(sort) : kSortDefault;
    k.grid = env_pos("RP_LOOKUP_GRID", 0);
    k.ticket = tick ? (is0(tick) ? 0 : 1) : -1;
    k.stagger = stag ? std::min(std::max(atoi(stag), 0), 64) : -1;
    k.ticket_grid = env_pos("RP_LOOKUP_TICKET_GRID", 0);
    k.tl_dump = getenv("RP_LK_TL_DUMP");
    k.lean_set = lean != nullptr;
    k.lean = !is0(lean);
    k.half_set = half != nullptr;
    k.half = num(half);
    k.fusefix = getenv_flag("RP_LOOKUP_FUSEFIX");
    k.stg_set = stg != nullptr;
    k.stg = num(stg);
    k.lh_set = getenv("RP_LOOKUP_LH") != nullptr;
    k.lh = env_pos("RP_LOOKUP_LH", 0);
    k.stghs = env_pos("RP_LOOKUP_STGHS", 8);
    k.debug = getenv_flag("RP_LOOKUP_DEBUG");
    k.prof_print = getenv_flag("RP_LK_PROF_PRINT");
    return k;
}

struct Ring {
    int device = 0;
    hipStream_t st = nullptr;
    uint32_t R = 100;
    // interned names (host mirror of JS `servers` keys + an id table)
    NameTable nt;
    std::vector<uint8_t> in_ring;
    std::vector<uint64_t> stamp;  // insertion stamp -> Object.keys order
    uint64_t next_stamp = 1;
    uint32_t server_count = 0;
    bool has_checksum = false;
    uint32_t checksum = 0;
    // ring arrays
    DevBuf<uint32_t> tok, own, tok2, own2, bstart;
    uint32_t M = 0;
    uint32_t bbits = 8;
    // packed lookup layout (valid while every interned id < 2^16)
    DevBuf<uint32_t> ent, pbstart;
    DevBuf<uint32_t> slow, nslow;  // deferred keys of the probe / compact kernels
    // The ticketed sorted tiles' counters: [0] tickets drawn, [1] workgroups that have left. Zeroed
    // once, when reserved; the last workgroup of every launch leaves both at 0. Like slow and
    // nslow they belong to one batch lookup at a time: a handle's lookups must not overlap on the
    // device (two streams without an order between them), or two launches share the tickets.
    DevBuf<uint32_t> tick;
    int ticket_per_cu = 0;  // k_lookupn_sorted_ticket<256, 3>'s workgroups a CU (0: not asked yet)
    bool packed = false;
    uint32_t pbits = 16;
    // compact lookup layout (the C2 hot path; valid while every interned id < 2^16)
    DevBuf<uint8_t> cent;
    DevBuf<uint32_t> cidx;
    DevBuf<uint32_t> cidxh;  // the hinted index (k_cindex_hint); valid when chint
    bool chint = false;
    bool chint_pending = false;  // the compact layout changed and the hinted index is not built yet
    bool compact = false;
    uint32_t ccb = 0, cob = 0, cfsh = 0;
    // the LDS-index layout (k_lookupn_lds, round 6), built by the first batch lookup after a change
    DevBuf<uint8_t> lent;
    DevBuf<uint4> lidx;
    bool lds = false, lds_pending = false;
    uint32_t lng = 0, llg = 0, lfb = 0;
    // checksum string + value
    DevBuf<uint8_t> d_inring;
    DevBuf<uint8_t> ck_buf;
    DevBuf<uint32_t> ck_out;  // [0] hash, [1] set
    // scratch
    DevBuf<uint32_t> ntok, nown, flag, pos, ids_dev, tmpk;
    DevBuf<uint64_t> tmp64;
    DevBuf<uint32_t> scalar;
    DevBuf<uint32_t> io_a, io_b;
    DevBuf<uint8_t> io_keys, io_cnt;
    // pinned, device-mapped rows / counts of the small host path (k_lookupn_small)
    uint32_t* pin_out = nullptr;
    uint8_t* pin_cnt = nullptr;
    uint32_t* pin_out_dev = nullptr;
    uint8_t* pin_cnt_dev = nullptr;
    DevBuf<uint64_t> io_off;
    // the lookup service (rp_ring_service): its pinned lines, stream, last answered seq
    SvcLines* svc = nullptr;
    SvcLines* svc_dev = nullptr;
    hipStream_t svc_st = nullptr;
    uint32_t svc_idle_ms = 0, svc_seq = 0;
    std::atomic<bool> svc_live{false};  // a wave launched and not yet stopped (counted in g_svc_live)
    std::recursive_mutex svc_mu;         // the service's lines and state (svc_lookup, svc_stop)
    bool svc_v2 = true;  // k_lookup_service3 (RP_RING_SVC=1: the round-4 kernel; read at rp_ring_service)
    DevBuf<uint4> svc_dt;       // the service's direct table (k_dt_build), built at its first launch after a change
    uint32_t svc_dtb = 0;       // its bucket bits; 0: none (ids past 16 bits, M > 2^22, RP_SVC_DT=0)
    bool svc_dt_valid = false;  // false after every ring change
    uint64_t svc_prof[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // RP_SVC_PROF: tick sums, path counts, calls
    // group keys by owner (handleOrProxyAll)
    DevBuf<uint32_t> grp_own, grp_key, grp_first, grp_dk, grp_dv, grp_rank;
    Scratch ws;
    LoadScratch load_ws;  // owner load / share
    RangeScratch range_ws;  // moved ranges
    HandoffScratch handoff_ws;  // hand-off plan
    RouteScratch route_ws;  // routing agreement
    uint32_t inring_n = 0;  // the ids d_inring covers (ring_compute_checksum copies in_ring at every change)

    RingView view() const {
        return RingView{tok.p, own.p, bstart.p, M, 32u - bbits};
    }
    PackedView pview() const { return PackedView{ent.p, pbstart.p, M, pbits}; }
    CompactView cview(const LookupKnobs& k) const {
        return CompactView{cent.p, cidx.p, M, ccb, cob, cfsh, cfsh == 0, (uint32_t)k.ablate,
                           (uint32_t)(3ull * ((uint64_t)M + kEnt3Pad + 6) + 16), (uint32_t)(8ull << (ccb - 3)),
                           k.wpred ? 1u : 0u, chint && k.hint ? cidxh.p : nullptr};
    }
};

// lookupN's replica count: the walk ends after np = min(nrep, server count) owners
// (lib/ring/index.js:159-162) and a row has W = max(nrep, 1) slots, whatever the servers.
struct Replicas {
    int np;
    uint32_t W;
};
static Replicas replicas(int32_t nrep, uint32_t servers) {
    return {(int)std::min<int64_t>(nrep, servers), nrep > 1 ? (uint32_t)nrep : 1u};
}

static uint32_t ring_intern(Ring& r, const char* s, uint32_t n) {
    const uint32_t id = r.nt.intern(s, n);
    if (id >= r.in_ring.size()) {
        r.in_ring.resize(id + 1, 0);
        r.stamp.resize(id + 1, 0);
    }
    return id;
}

static uint32_t choose_bbits(uint32_t M) {
    // ~4 tokens per bucket: a bounded 2-3 step search inside one or two cache lines.
    uint32_t b = 8;
    while (b < 22 && (1ull << (b + 2)) < M) b++;
    return b;
}

// The compact layout (CompactView): 2^cb buckets with cb = floor(log2 M), owner ids in ob bits,
// fingerprints of 24 - ob bits. Not built for tiny rings, more than 2^16 interned names, or a
// bucket of more than 15 tokens (caller hashFunc values that collide); the packed / wide
// layouts serve those.
static void ring_build_compact(Ring& r) {
    r.compact = false;
    if (r.M < 64) return;
    uint32_t ob = 1;
    while ((1ull << ob) < r.nt.size()) ob++;
    if (ob > 16) return;
    uint32_t cb = 3;
    while (cb < 24 && (2ull << cb) <= r.M) cb++;
    if (const char* d = getenv("RP_COMPACT_CB_DELTA")) {  // A/B knob: bucket density
        const int c = (int)cb + atoi(d);
        cb = (uint32_t)(c < 3 ? 3 : c > 24 ? 24 : c);
    }
    const uint32_t rb = 32 - cb, fb = 24 - ob;
    const uint32_t fsh = fb >= rb ? 0 : rb - fb;
    const uint64_t nbk = 1ull << cb, ngroups = nbk >> 3;
    r.tmpk.reserve(nbk + 1);
    hipLaunchKernelGGL(k_bucket_index, dim3(grid_for(nbk + 1, 256)), dim3(256), 0, r.st, r.tok.p, r.M, cb, r.tmpk.p);
    r.cidx.reserve(2 * ngroups);
    r.scalar.reserve(1);
    RP_HIP(hipMemsetAsync(r.scalar.p, 0, sizeof(uint32_t), r.st));
    hipLaunchKernelGGL(k_cindex, dim3(grid_for(ngroups, 256)), dim3(256), 0, r.st, r.tmpk.p, (uint32_t)ngroups,
                       r.cidx.p, r.scalar.p);
    r.cent.reserve(3ull * ((uint64_t)r.M + kEnt3Pad + 6) + 16);
    hipLaunchKernelGGL(k_pack3, dim3(grid_for((uint64_t)r.M + kEnt3Pad + 6, 256)), dim3(256), 0, r.st, r.tok.p,
                       r.own.p, r.M, cb, ob, fsh, r.cent.p);
    RP_HIP(hipGetLastError());
    if (read_u32(r.scalar.p, r.st) != 0) return;
    // the hinted index of the lean lookupN(3) (needs bucket bits >= 11: 8 prediction bits below)
    // is built by the first batch lookup that reads it (ring_build_hint): ~1 ms at C2, which a
    // per-call mutation (addServer / removeServer) should not pay
    r.chint = false;
    r.chint_pending = 32 - cb >= 8 && r.M < (1u << 30);
    r.lds = false;
    r.lds_pending = ob <= 14;
    r.compact = true;
    r.ccb = cb;
    r.cob = ob;
    r.cfsh = fsh;
}

static void ring_build_hint(Ring& r) {
    r.chint_pending = false;
    r.chint = false;
    const uint32_t cb = r.ccb;
    const uint64_t nbk = 1ull << cb, ngroups = nbk >> 3;
    r.tmpk.reserve(nbk + 1);
    hipLaunchKernelGGL(k_bucket_index, dim3(grid_for(nbk + 1, 256)), dim3(256), 0, r.st, r.tok.p, r.M, cb, r.tmpk.p);
    r.cidxh.reserve(2 * ngroups);
    RP_HIP(hipMemsetAsync(r.scalar.p, 0, sizeof(uint32_t), r.st));
    hipLaunchKernelGGL(k_cindex_hint, dim3(grid_for(ngroups, 256)), dim3(256), 0, r.st, r.tok.p, r.tmpk.p, r.M, cb,
                       (uint32_t)ngroups, r.cidxh.p, r.scalar.p);
    RP_HIP(hipGetLastError());
    r.chint = read_u32(r.scalar.p, r.st) == 0;
}

// The LDS-index layout (LdsView): ng = the power of two nearest M / 126 (about 4.5 tokens a bucket),
// 64..8,192 groups; not built past 5.5 tokens a bucket at 8,192 groups (M > 1.26 M), for owner ids
// past 14 bits (fingerprints under 10 bits), or when a group's base does not fit its int16 delta.
static void ring_build_lds(Ring& r) {
    r.lds_pending = false;
    r.lds = false;
    uint32_t lg = 6;
    while (lg < 13 && (1ull << lg) * 126ull < r.M) lg++;
    const uint64_t ng = 1ull << lg;
    if ((double)r.M / (28.0 * (double)ng) > 5.5 || r.cob > 14) return;
    const uint32_t fb = 24u - r.cob;
    r.lidx.reserve(ng);
    RP_HIP(hipMemsetAsync(r.scalar.p, 0, sizeof(uint32_t), r.st));
    hipLaunchKernelGGL(k_lidx_build, dim3(grid_for(ng, 256)), dim3(256), 0, r.st, r.tok.p, r.M, lg, (uint32_t)ng,
                       r.lidx.p, r.scalar.p);
    r.lent.reserve(3ull * ((uint64_t)r.M + kEnt3Pad + 6) + 16);
    hipLaunchKernelGGL(k_lpack3, dim3(grid_for((uint64_t)r.M + kEnt3Pad + 6, 256)), dim3(256), 0, r.st, r.tok.p,
                       r.own.p, r.M, lg, fb, r.cob, r.lent.p);
    RP_HIP(hipGetLastError());
    if (read_u32(r.scalar.p, r.st) != 0) return;
    r.lng = (uint32_t)ng;
    r.llg = lg;
    r.lfb = fb;
    r.lds = true;
}

static void ring_rebuild_index(Ring& r) {
    r.svc_dt_valid = false;
    r.bbits = choose_bbits(r.M);
    const uint64_t nbk = (1ull << r.bbits) + 1;
    r.bstart.reserve(nbk);
    hipLaunchKernelGGL(k_bucket_index, dim3(grid_for(nbk, 256)), dim3(256), 0, r.st, r.tok.p, r.M, r.bbits,
                       r.bstart.p);
    RP_HIP(hipGetLastError());
    // packed layout: 2^B >= M (about one token per bucket, so the 4 entries at the bucket
    // start usually hold the answer) and every interned id < 2^B; B <= 24 (64 MB index)
    uint32_t B = 8;
    while (B < 24 && ((1ull << B) < r.M || (1ull << B) < r.nt.size())) B++;
    r.packed = (1ull << B) >= r.nt.size();
    if (r.packed) {
        r.pbits = B;
        r.ent.reserve((uint64_t)r.M + kEntPad);
        r.pbstart.reserve((1ull << B) + 1);
        hipLaunchKernelGGL(k_pack, dim3(grid_for((uint64_t)r.M + kEntPad, 256)), dim3(256), 0, r.st, r.tok.p,
                           r.own.p, r.M, B, r.ent.p);
        hipLaunchKernelGGL(k_bucket_index, dim3(grid_for((1ull << B) + 1, 256)), dim3(256), 0, r.st, r.tok.p, r.M,
                           B, r.pbstart.p);
        RP_HIP(hipGetLastError());
    }
    ring_build_compact(r);
}

// Device replica tokens for server ids (or caller tokens), sorted stably by token.
static uint64_t ring_make_tokens(Ring& r, const std::vector<uint32_t>& sel_ids, const std::vector<uint32_t>* custom) {
    const uint64_t K = (uint64_t)sel_ids.size() * r.R;
    RP_REQUIRE(K < (1ull << 31), "too many replica points in one batch");
    r.ntok.reserve(K + 1);
    r.nown.reserve(K + 1);
    r.ids_dev.reserve(sel_ids.size() + 1);
    RP_HIP(hipMemcpyAsync(r.ids_dev.p, sel_ids.data(), sizeof(uint32_t) * sel_ids.size(), hipMemcpyHostToDevice,
                          r.st));
    if (custom) {
        RP_HIP(hipMemcpyAsync(r.ntok.p, custom->data(), sizeof(uint32_t) * K, hipMemcpyHostToDevice, r.st));
        hipLaunchKernelGGL(k_expand_owner, dim3(grid_for(K, 256)), dim3(256), 0, r.st, r.ids_dev.p,
                           (uint32_t)sel_ids.size(), r.R, r.nown.p);
    } else {
        hipLaunchKernelGGL(k_replica_tokens, dim3(grid_for(K, 256)), dim3(256), 0, r.st, r.nt.d_bytes.p, r.nt.d_noff.p,
                           r.ids_dev.p, (uint32_t)sel_ids.size(), r.R, r.ntok.p, r.nown.p);
    }
    RP_HIP(hipGetLastError());
    return K;
}

static void ring_apply_adds(Ring& r, const std::vector<uint32_t>& add_ids, const std::vector<uint32_t>* custom) {
    if (add_ids.empty()) return;
    const uint64_t K = ring_make_tokens(r, add_ids, custom);
    radix_sort_pairs(r.ntok.p, r.nown.p, K, 0, 32, r.st, r.ws);
    r.flag.reserve(K + 1);
    r.pos.reserve(K + 1);
    hipLaunchKernelGGL(k_mark_new, dim3(grid_for(K, 256)), dim3(256), 0, r.st, r.ntok.p, (uint32_t)K, r.tok.p, r.M,
                       r.flag.p);
    RP_HIP(hipGetLastError());
    scan_exclusive_u32(r.flag.p, r.pos.p, K, r.st, r.ws);
    const uint32_t Kp = read_u32(r.pos.p + K, r.st);
    r.tmpk.reserve((uint64_t)Kp + 1);
    r.ws.c.reserve((uint64_t)Kp + 1);
    hipLaunchKernelGGL(k_compact_pairs, dim3(grid_for(K, 256)), dim3(256), 0, r.st, r.ntok.p, r.nown.p, r.flag.p,
                       r.pos.p, (uint32_t)K, r.tmpk.p, r.ws.c.p);
    const uint64_t nM = (uint64_t)r.M + Kp;
    RP_REQUIRE(nM < 0xFFFFFFF0ull, "ring too large");
    r.tok2.reserve(nM + 1);
    r.own2.reserve(nM + 1);
    hipLaunchKernelGGL(k_merge, dim3(grid_for(nM, 256)), dim3(256), 0, r.st, r.tok.p, r.own.p, r.M, r.tmpk.p,
                       r.ws.c.p, Kp, r.tok2.p, r.own2.p);
    RP_HIP(hipGetLastError());
    r.tok.swap(r.tok2);
    r.own.swap(r.own2);
    r.M = (uint32_t)nM;
}

static void ring_apply_removes(Ring& r, const std::vector<uint32_t>& rem_ids, const std::vector<uint32_t>* custom) {
    if (rem_ids.empty() || r.M == 0) return;
    const uint64_t K = ring_make_tokens(r, rem_ids, custom);
    r.flag.reserve((uint64_t)r.M + 1);
    r.pos.reserve((uint64_t)r.M + 1);
    hipLaunchKernelGGL(k_fill_u32, dim3(grid_for(r.M, 256)), dim3(256), 0, r.st, r.flag.p, (uint64_t)r.M, 1u);
    hipLaunchKernelGGL(k_mark_del, dim3(grid_for(K, 256)), dim3(256), 0, r.st, r.ntok.p, K, r.tok.p, r.M, r.flag.p);
    RP_HIP(hipGetLastError());
    scan_exclusive_u32(r.flag.p, r.pos.p, r.M, r.st, r.ws);
    const uint32_t nM = read_u32(r.pos.p + r.M, r.st);
    r.tok2.reserve((uint64_t)nM + 1);
    r.own2.reserve((uint64_t)nM + 1);
    hipLaunchKernelGGL(k_compact_pairs, dim3(grid_for(r.M, 256)), dim3(256), 0, r.st, r.tok.p, r.own.p, r.flag.p,
                       r.pos.p, r.M, r.tok2.p, r.own2.p);
    RP_HIP(hipGetLastError());
    r.tok.swap(r.tok2);
    r.own.swap(r.own2);
    r.M = nM;
}

// HashRing.computeChecksum (lib/ring/index.js:96-105) on the device:
// hash32(Object.keys(servers).sort().join(';')), names in byte order (NameTable::sort).
static void ring_compute_checksum(Ring& r) {
    r.nt.sort(r.st, r.ws);
    const uint32_t n = r.nt.size();
    r.d_inring.reserve((uint64_t)n + 1);
    if (n) RP_HIP(hipMemcpyAsync(r.d_inring.p, r.in_ring.data(), n, hipMemcpyHostToDevice, r.st));
    r.inring_n = n;
    r.flag.reserve((uint64_t)n + 1);
    r.pos.reserve((uint64_t)n + 1);
    r.ck_buf.reserve(r.nt.h_bytes.size() + n + 16);
    r.ck_out.reserve(2);
    if (n) {
        hipLaunchKernelGGL(k_ck_len, dim3(grid_for(n, 256)), dim3(256), 0, r.st, r.nt.sorted.p, n, r.d_inring.p,
                           r.nt.d_noff.p, r.flag.p);
        scan_exclusive_u32(r.flag.p, r.pos.p, n, r.st, r.ws);
        hipLaunchKernelGGL(k_ck_scatter, dim3(grid_for((uint64_t)n * 64, 256)), dim3(256), 0, r.st, r.nt.sorted.p, n,
                           r.d_inring.p, r.nt.d_bytes.p, r.nt.d_noff.p, r.pos.p, r.ck_buf.p);
        RP_HIP(hipGetLastError());
        hash_long(r.ck_buf.p, 0, r.pos.p + n, nullptr, r.ck_out.p, r.st);
    } else {
        hash_long(r.ck_buf.p, 0, nullptr, nullptr, r.ck_out.p, r.st);  // "" (empty ring)
    }
    uint32_t v[2];
    RP_HIP(hipMemcpyAsync(v, r.ck_out.p, sizeof v, hipMemcpyDeviceToHost, r.st));
    RP_HIP(hipStreamSynchronize(r.st));
    scratch_check(r.ws, r.st);
    r.checksum = v[0];
    r.has_checksum = true;
}

// ------------------------------------------------------------------- batch lookup launch
// launch_lookupn (below) tries, in this order: the LDS-index kernel, the wave-specialised kernel,
// the compact layout's sorted / lean / round-1 kernels, the packed window probe, and then the
// generic kernels over the packed or the wide view.

// f(Int<N>{}) for the N = 1..4 owners a row the tiled kernels are built for
template <int N>
using Int = std::integral_constant<int, N>;
template <class F>
static void with_need(int need, F&& f) {
    switch (need) {
        case 1: f(Int<1>{}); break;
        case 2: f(Int<2>{}); break;
        case 3: f(Int<3>{}); break;
        default: f(Int<4>{}); break;
    }
}

// A key stream on the device, as the kernels take it: key bytes (stride > 0: key i is
// keys[i * stride .. + stride), else keys[off[i] .. off[i + 1])) or, with `hashes`, the key hashes.
struct DevKeys {
    const uint8_t* keys;
    const uint64_t* off;
    uint32_t stride;
    const uint32_t* hashes;
    // 36-byte keys at a 4-byte aligned address: what the kernels' fixed forms read as nine dwords
    bool fixed36() const { return !hashes && stride == 36 && ((reinterpret_cast<uintptr_t>(keys) & 3) == 0); }
    // the stream from key k0 on (a chunk of a pass); the buffers the form does not read are null
    DevKeys from(uint64_t k0) const {
        return {hashes ? nullptr : (stride ? keys + k0 * stride : keys), (!hashes && !stride) ? off + k0 : nullptr, stride,
                hashes ? hashes + k0 : nullptr};
    }
};

// The kernels over any view: 36-byte keys at a 4-byte-aligned address in registers
// (k_lookupn_fixed), every other key form and caller hashes per thread (k_lookupn_generic).
// `ablate`: LookupKnobs::ablate.
template <class View>
static void launch_lookupn_view(const View& rv, const uint8_t* keys, const uint64_t* off, uint32_t stride,
                                const uint32_t* hashes, uint64_t n, int np, uint32_t W, uint32_t* out,
                                uint8_t* counts, hipStream_t st, int ablate) {
    const bool fixed36 = DevKeys{keys, off, stride, hashes}.fixed36();
    const int need = np <= 0 ? 1 : np;
    const auto fixed = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid_for(n, kLkThreads, 256 * 8)), dim3(kLkThreads), 0, st, keys, n, rv, np, W,
                           out, counts);
    };
    const auto generic = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid_for(n, 256, 256 * 8)), dim3(256), 0, st, keys, off, stride, hashes, n, rv,
                           np, W, out, counts);
    };
    if (fixed36 && W <= 4 && need <= 4 && need > 1 && ablate == 1)
        fixed(k_lookupn_fixed<36, 4, View, 1>);
    else if (fixed36 && W <= 4 && need <= 4 && need > 1 && ablate == 2)
        fixed(k_lookupn_fixed<36, 4, View, 2>);
    else if (fixed36 && need == 1 && W == 1)
        fixed(k_lookupn_fixed<36, 1, View>);
    else if (fixed36 && need <= 4 && W <= 4)
        fixed(k_lookupn_fixed<36, 4, View>);
    else if (fixed36 && need <= 8 && W <= 8)
        fixed(k_lookupn_fixed<36, 8, View>);
    else if (need == 1)
        generic(k_lookupn_generic<1, View>);
    else if (need <= 4)
        generic(k_lookupn_generic<4, View>);
    else if (need <= 8)
        generic(k_lookupn_generic<8, View>);
    else
        generic(k_lookupn_generic<0, View>);
    RP_HIP(hipGetLastError());
}

// A batch of 36-byte keys at a 4-byte-aligned address: what the tiled and the probe kernels take.
struct Batch36 {
    const uint8_t* keys;
    uint64_t n;
    int np, need;  // need = max(np, 1)
    uint32_t W;
    uint32_t* out;
    uint8_t* counts;
    hipStream_t st;
};

// The end of every tiled path. The tile kernels left the keys they could not finish in `nlists`
// lists, one per TK-key tile from the first key on: finish those exactly (`fix`; the compact path
// turns it off), print their census under RP_LOOKUP_DEBUG through line(keys done, deferred,
// overflowed lists, the nlists + extra words of r.nslow), and send the keys past `done`, the
// partial last tile, through the wide view.
template <class Line>
static void lookupn_tiles_end(Ring& r, const LookupKnobs& k, const Batch36& b, uint64_t nlists, uint64_t TK,
                              uint64_t done, bool fix, uint64_t extra, Line&& line) {
    if (fix) {
        const CompactFixView fv{r.tok.p, r.own.p, r.cidx.p, r.view(), r.M, r.ccb};
        const uint64_t fthreads = nlists * kSlowPerTile;
        hipLaunchKernelGGL((k_lookupn_fix_tiles<CompactFixView>), dim3((unsigned)((fthreads + 255) / 256)), dim3(256),
                           0, b.st, b.keys, fv, b.np, b.W, b.out, b.counts, r.slow.p, r.nslow.p, nlists, (uint32_t)TK);
    }
    RP_HIP(hipGetLastError());
    if (k.debug) {
        std::vector<uint32_t> c(nlists + extra);
        RP_HIP(hipMemcpyAsync(c.data(), r.nslow.p, 4 * (nlists + extra), hipMemcpyDeviceToHost, b.st));
        RP_HIP(hipStreamSynchronize(b.st));
        uint64_t tot = 0, over = 0;
        for (uint64_t t = 0; t < nlists; t++) {
            tot += c[t];
            over += c[t] > kSlowPerTile;
        }
        line((unsigned long long)done, (unsigned long long)tot, (unsigned long long)over, c.data());
    }
    if (done < b.n)
        launch_lookupn_view(r.view(), b.keys + done * 36, nullptr, 36, nullptr, b.n - done, b.np, b.W,
                            b.out + done * b.W, b.counts ? b.counts + done : nullptr, b.st, k.ablate);
}

// The LDS-index kernel (round 6; RP_LOOKUP_LDS=0 keeps the lean kernel, 1 forces this one)
static bool lookupn_lds(Ring& r, const LookupKnobs& k, const Batch36& b) {
    if (!k.lds || b.n < 64ull * 8 || k.ablate_set) return false;
    if (r.lds_pending) ring_build_lds(r);
    if (!r.lds) return false;
    RP_REQUIRE(b.n < (1ull << 32), "lookupn: at most 2^32-1 keys per call");
    constexpr int KPL = 8;
    const uint64_t TK = 64ull * KPL, nwt = b.n / TK;
    r.slow.reserve(nwt * kSlowPerTile + 1);
    r.nslow.reserve(nwt + 1);
    const unsigned g = (unsigned)std::min<uint64_t>(k.lds_grid ? k.lds_grid : (uint64_t)cu_count(r.device),
                                                    (nwt + kLdsThreads / 64 - 1) / (kLdsThreads / 64));
    const LdsView lv{r.lent.p, r.lidx.p, r.M, r.lng, r.llg, r.lfb, r.cob,
                     (uint32_t)(3ull * ((uint64_t)r.M + kEnt3Pad + 6) + 16)};
    const auto tiles = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(g), dim3(kLdsThreads), 0, b.st, b.keys, nwt, lv, b.out, b.counts, r.slow.p,
                           r.nslow.p);
    };
    if (b.need == 3 && k.lds_abl) {  // diagnostics: time ablations (results wrong)
        switch (k.lds_abl) {
            case 1: tiles(k_lookupn_lds<KPL, 3, 0, 1>); break;
            case 2: tiles(k_lookupn_lds<KPL, 3, 0, 2>); break;
            case 3: tiles(k_lookupn_lds<KPL, 3, 0, 3>); break;
            case 4: tiles(k_lookupn_lds<KPL, 3, 0, 4>); break;
            default: tiles(k_lookupn_lds<KPL, 3, 0, 7>); break;
        }
    } else {
        with_need(b.need, [&](auto need) {
            constexpr int N = decltype(need)::value;
            if (k.lds_stg)
                tiles(k_lookupn_lds<KPL, N, 1, 0>);
            else
                tiles(k_lookupn_lds<KPL, N, 0, 0>);
        });
    }
    RP_HIP(hipGetLastError());
    lookupn_tiles_end(r, k, b, nwt, TK, nwt * TK, true, 0,
                      [&](auto done, auto tot, auto over, const uint32_t*) {
                          fprintf(stderr, "[rp] lds lookupN: %llu keys, %llu deferred, %llu overflowed tiles (ng %u fb %u ob %u)\n",
                                  done, tot, over, r.lng, r.lfb, r.cob);
                      });
    return true;
}

// The wave-specialised kernel (round 6, A/B): RP_LOOKUP_WS = "NP:NC" producer and consumer
// waves a workgroup (1:3, 2:6, 1:7, 4:12, 2:2, 1:15, 2:14; "1" = 1:3)
static bool lookupn_ws(Ring& r, const LookupKnobs& k, const Batch36& b, const CompactView& cv) {
    const uint64_t n = b.n;
    if (!k.ws || b.need != 3 || k.kpl_set || cv.ablate != 0 || n < 512ull * 4 || n * 12ull >= (1ull << 31))
        return false;
    const int wnp = k.ws_np, wnc = k.ws_nc;
    constexpr uint64_t TK = 512;
    const uint64_t nwt = n / TK;
    r.slow.reserve(nwt * kSlowPerTile + 1);
    r.nslow.reserve(nwt + 2);
    uint32_t* err = r.nslow.p + nwt + 1;
    RP_HIP(hipMemsetAsync(err, 0, 4, b.st));
    const uint64_t nwg = (nwt + (uint64_t)wnc - 1) / (uint64_t)(wnc > 0 ? wnc : 1);
    // workgroups a CU: 16 waves (<= 128 VGPRs), and the LDS (an 18-KB key tile a producer,
    // kWsSlots 2-KB ring slots and a 768-B list a consumer)
    const uint64_t lds_wg = (uint64_t)wnp * 18432 + (uint64_t)wnc * (kWsSlots * 2048 + 780);
    const uint64_t per_cu = wnp + wnc > 0 ? std::max<uint64_t>(1, std::min<uint64_t>(16 / (uint64_t)(wnp + wnc), 163840 / lds_wg)) : 1;
    const unsigned g = (unsigned)std::min<uint64_t>(nwg, k.ws_grid ? k.ws_grid : (uint64_t)cu_count(r.device) * per_cu);
    // the shapes built; RP_LOOKUP_WS_ABL = 1 | 2 (diagnostics) takes an ablated 4:12
    using Kernel = decltype(&k_lookupn_ws<1, 3>);
    static const struct { int np, nc, abl; Kernel kern; } shapes[] = {
        {1, 3, 0, k_lookupn_ws<1, 3>},      {2, 6, 0, k_lookupn_ws<2, 6>},      {1, 7, 0, k_lookupn_ws<1, 7>},
        {4, 12, 1, k_lookupn_ws<4, 12, 1>}, {4, 12, 2, k_lookupn_ws<4, 12, 2>}, {4, 12, 0, k_lookupn_ws<4, 12>},
        {2, 2, 0, k_lookupn_ws<2, 2>},      {1, 15, 0, k_lookupn_ws<1, 15>},    {2, 14, 0, k_lookupn_ws<2, 14>}};
    Kernel kern = nullptr;
    for (const auto& s : shapes)
        if (!kern && s.np == wnp && s.nc == wnc && (s.abl == 0 || s.abl == k.ws_abl)) kern = s.kern;
    RP_REQUIRE(kern, "RP_LOOKUP_WS: one of 1:3, 2:6, 1:7, 4:12, 2:2, 1:15, 2:14");
    hipLaunchKernelGGL(kern, dim3(g), dim3((wnp + wnc) * 64), 0, b.st, b.keys, nwt, cv, b.out, (uint32_t)(n * 12ull), b.counts,
                       r.slow.p, r.nslow.p, err);
    RP_HIP(hipGetLastError());
    lookupn_tiles_end(r, k, b, nwt, TK, nwt * TK, true, 2,
                      [&](auto done, auto tot, auto over, const uint32_t* c) {
                          fprintf(stderr, "[rp] ws lookupN %d:%d: %llu keys, %llu deferred, %llu overflowed wave-tiles, err %u\n", wnp,
                                  wnc, done, tot, over, c[nwt + 1]);
                      });
    return true;
}

// The compact layout's own kernels: whole sorted tiles first (lookupN(3) only), whole tiles of
// the lean kernel (RP_LOOKUP_LEAN=0: the round-1 kernel) after them.
static void lookupn_compact(Ring& r, const LookupKnobs& k, const Batch36& b, const CompactView& cv) {
    const uint64_t n = b.n;
    const int need = b.need, np = b.np;
    const hipStream_t st = b.st;
    // lookupN(3) (the C2 bench): 8 keys per lane, staged through LDS in four slices (0.925-0.926
    // against 0.962-0.970 ms for 4 keys per lane; two slices 0.926-0.932; 6 keys per lane
    // 0.956-0.959; profiles/r02/ab_lookup_lean.json); the other widths 4 keys per lane.
    // RP_LOOKUP_KPL / RP_LOOKUP_HALF (slices: 2, 4) override (A/B).
    int kpl = k.kpl_set ? k.kpl : (need == 3 ? 8 : 4);
    if (kpl != 1 && kpl != 2 && !((kpl == 3 || kpl == 8) && need == 3)) kpl = 4;  // the instantiated tiles
    // The sorted-tile kernel (RP_LOOKUP_SORT = 256 (default) | 512 | 1024 threads, 0 = off): only where
    // the lean <8, 3, 4> kernel runs by default (lookupN(3) over the hinted index, no other
    // RP_LOOKUP_* shape knob). It takes the whole tiles of 8 x threads keys; the rest goes on
    // to the lean kernel's 2,048-key tiles and the generic kernel as before, and one fix pass
    // covers both (the sorted kernel defers into the same 2,048-key lists).
    int sort_t = k.sort_t;
    RP_REQUIRE(sort_t == 0 || sort_t == 256 || sort_t == 512 || sort_t == 1024, "RP_LOOKUP_SORT: one of 0, 256, 512, 1024");
    if (need != 3 || !cv.idxh || cv.ablate != 0 || n < 8ull * (uint64_t)sort_t || k.kpl_set || k.half_set ||
        k.lean_set || k.stg_set || k.lh_set || k.fusefix)
        sort_t = 0;
    const uint64_t stiles = sort_t ? n / (8ull * (uint64_t)sort_t) : 0;
    const uint64_t s0 = stiles * 8ull * (uint64_t)sort_t;  // keys the sorted kernel takes
    const uint64_t t0 = s0 / 2048;                         // their 2,048-key lists
    if (!sort_t && n < (uint64_t)kLkThreads * kpl) kpl = 4;  // at least one whole tile
    const uint64_t TK = (uint64_t)kLkThreads * kpl;
    const uint64_t ntiles = (n - s0) / TK, done = s0 + ntiles * TK;
    r.slow.reserve((t0 + ntiles) * kSlowPerTile + 1);
    r.nslow.reserve(t0 + ntiles + 1);
    // The 256-thread tiles by ticket (RP_LOOKUP_TICKET; an explicit RP_LOOKUP_GRID names the
    // strided kernel): the grid is what is resident, the CUs times the workgroups a CU of the
    // occupancy query, capped at the tile count.
    const bool ticket = stiles && sort_t == 256 && !k.grid && (k.ticket < 0 ? kTicketDefault : k.ticket == 1);
    unsigned sg = 0;
    int stag16 = 0;
    if (ticket) {
        if (!r.tick.p) {
            r.tick.reserve(2);
            RP_HIP(hipMemsetAsync(r.tick.p, 0, 2 * sizeof(uint32_t), st));
            RP_HIP(hipStreamSynchronize(st));  // once a handle: later calls may come on other streams
        }
        if (!r.ticket_per_cu) {
            int nbl = 0;
            RP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbl, reinterpret_cast<const void*>(k_lookupn_sorted_ticket<256, 3>), 256, 0));
            r.ticket_per_cu = std::max(nbl, 1);
        }
        const uint64_t cus = (uint64_t)cu_count(r.device);
        sg = (unsigned)(k.ticket_grid ? std::min<uint64_t>(k.ticket_grid, 1u << 20) : std::min<uint64_t>(cus * (uint64_t)r.ticket_per_cu, stiles));
        // the stagger in s_sleep(16) = 1,024 clocks a step: stag16 / 16 of a tile time (kSortedTileUs)
        stag16 = k.stagger < 0 ? kStaggerDefault : k.stagger;
        int khz = 0;
        if (stag16) (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, r.device);
        const uint32_t naps = (uint32_t)((uint64_t)stag16 * kSortedTileUs * (uint64_t)(khz > 0 ? khz / 1000 : 2400) / (16u * 1024u));
        // slot j of a CU: workgroups are dealt over the CUs before a CU gets its next one
        // (profiles/ticket_tiles/), so j = blockIdx.x / CUs
        hipLaunchKernelGGL((k_lookupn_sorted_ticket<256, 3>), dim3(sg), dim3(256), 0, st, b.keys, stiles, cv, b.out, b.counts,
                           r.slow.p, r.nslow.p, r.tick.p, naps, (uint32_t)cus);
        RP_HIP(hipGetLastError());
    } else if (stiles) {
        // workgroups, tiles strided over them (2^26 C2 keys, profiles/sorted_tiles/grid_sweep.txt):
        // 256 threads 0.842 ms at 4096 (2048: 0.877, 8192: 0.845, 12288: 0.850); 512 threads 0.890
        // at 8192 (1024-4096: 0.93-0.95); 1024 threads 0.997 at 512-1024. RP_LOOKUP_GRID overrides (A/B).
        sg = grid_for(stiles, 1, (unsigned)(k.grid ? k.grid : sort_t == 256 ? 4096u : sort_t == 512 ? 8192u : 1024u));
        const auto sorted = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(sg), dim3(sort_t), 0, st, b.keys, stiles, cv, b.out, b.counts, r.slow.p, r.nslow.p);
        };
        if (sort_t == 256)
            sorted(k_lookupn_sorted<256, 3>);
        else if (sort_t == 512)
            sorted(k_lookupn_sorted<512, 3>);
        else
            sorted(k_lookupn_sorted<1024, 3>);
        RP_HIP(hipGetLastError());
    }
    const bool lean = k.lean;  // A/B: RP_LOOKUP_LEAN=0 = round-1 kernel
    // workgroups, tiles strided over them: the lean kernel at 4096 (4 rounds of the 1024 that
    // fit, 8 tiles each at C2) ran 0.905-0.911 ms against 0.926-0.930 at 2048 (3072: 0.917;
    // 5120-16384: 0.908-0.914; profiles/r02/ab_lookup_grid.json). RP_LOOKUP_GRID overrides (A/B).
    const unsigned g = grid_for(ntiles, 1, (unsigned)(k.grid ? k.grid : lean ? 4096u : 2048u));
    const int half = k.half_set ? k.half : (kpl == 8 ? 4 : 0);
    const CompactFixView fv{r.tok.p, r.own.p, r.cidx.p, r.view(), r.M, r.ccb};
    // deferred keys finished by the lean kernel's own workgroups (A/B): only <8, 3, 4>
    const bool fuse = k.fusefix && lean && half == 4 && kpl == 8 && need == 3 && cv.ablate != 3;
    const bool stg1 = k.stg == 1 && lean && half == 4 && kpl == 8 && need == 3 && !fuse;
    // RP_LOOKUP_STG=2: asm DMA ring (RP_LOOKUP_STGHS = 4 | 8 key slices; RP_LOOKUP_LH = 1 | 2)
    const bool stg2 = lean && kpl == 8 && need == 3 && !fuse && k.stg == 2;
    const int lh = (lean && (half == 4 || stg2) && kpl == 8 && need == 3 && !fuse)
                       ? (int)(k.lh ? k.lh : (stg2 ? 2u : 1u)) : 1;
    const int stghs = (int)k.stghs;
    // the lean kernel's share: the keys after the sorted tiles, and their lists
    const auto tiles = [&](auto kern, auto... fix) {
        hipLaunchKernelGGL(kern, dim3(g), dim3(kLkThreads), 0, st, b.keys + s0 * 36, ntiles, cv, b.out + s0 * b.W,
                           b.counts ? b.counts + s0 : nullptr, r.slow.p + t0 * kSlowPerTile, r.nslow.p + t0, fix...);
    };
    const auto run = [&](auto keys_per_lane, auto owners) {
        constexpr int KPL = decltype(keys_per_lane)::value, NEED = decltype(owners)::value;
        if (!lean) return tiles(k_lookupn_compact<KPL, NEED>);
        if constexpr (KPL == 8 && NEED == 3) {  // the staging variants exist for this tile only
            if (stg2 && stghs == 8 && lh == 1) return tiles(k_lookupn_lean<8, 3, 8, false, 2, 1>, fv, np);
            if (stg2 && stghs == 8) return tiles(k_lookupn_lean<8, 3, 8, false, 2, 2>, fv, np);
            if (stg2) return tiles(k_lookupn_lean<8, 3, 4, false, 2, 2>, fv, np);
            if (stg1 && lh == 2) return tiles(k_lookupn_lean<8, 3, 4, false, 1, 2>, fv, np);
            if (lh == 2) return tiles(k_lookupn_lean<8, 3, 4, false, 0, 2>, fv, np);
            if (stg1) return tiles(k_lookupn_lean<8, 3, 4, false, 1>, fv, np);
        }
        if (half == 4 && KPL % 4 == 0 && fuse) return tiles(k_lookupn_lean<KPL, NEED, (KPL % 4 == 0 ? 4 : 1), true>, fv, np);
        if (half == 4 && KPL % 4 == 0) return tiles(k_lookupn_lean<KPL, NEED, (KPL % 4 == 0 ? 4 : 1)>, fv, np);
        if (half == 2 && KPL % 2 == 0) return tiles(k_lookupn_lean<KPL, NEED, (KPL % 2 == 0 ? 2 : 1)>, fv, np);
        return tiles(k_lookupn_lean<KPL, NEED>, fv, np);
    };
    if (ntiles == 0) {  // the sorted kernel took every whole tile
    } else if (kpl == 1) {
        with_need(need, [&](auto owners) { run(Int<1>{}, owners); });
    } else if (kpl == 2) {
        with_need(need, [&](auto owners) { run(Int<2>{}, owners); });
    } else if (kpl == 8 && need == 3) {
        run(Int<8>{}, Int<3>{});
    } else if (kpl == 3 && need == 3) {
        run(Int<3>{}, Int<3>{});
    } else {
        with_need(need, [&](auto owners) { run(Int<4>{}, owners); });
    }
#ifdef RP_LK_PROF
    if (k.prof_print) {
        unsigned long long v[10];
        RP_HIP(hipStreamSynchronize(st));
        RP_HIP(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_lk_prof), sizeof v));
        const double nw = (double)(v[6] ? v[6] : 1);
        fprintf(stderr,
                "[rp] lean phase cycles per wave-tile (%llu): keys-arrive %.0f hash-all %.0f idx %.0f win1+loop %.0f "
                "finish2 %.0f barrier+store %.0f\n",
                v[6], v[0] / nw, v[1] / nw, v[2] / nw, v[3] / nw, v[4] / nw, v[5] / nw);
        memset(v, 0, sizeof v);
        RP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_lk_prof), v, sizeof v));
        if (stiles) {
            RP_HIP(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_sk_prof), sizeof v));
            const double sw = (double)(v[6] ? v[6] : 1);
            fprintf(stderr,
                    "[rp] sorted<%d> phase cycles per wave-tile (%llu): keys+hash %.0f sort+deal %.0f idx+win-issue %.0f "
                    "win1+loop %.0f finish2 %.0f barrier+store %.0f\n",
                    sort_t, v[6], v[0] / sw, v[1] / sw, v[2] / sw, v[3] / sw, v[4] / sw, v[5] / sw);
            memset(v, 0, sizeof v);
            RP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_sk_prof), v, sizeof v));
        }
    }
#endif
#ifdef RP_LK_TL
    if (k.tl_dump && stiles) {  // the sorted launch's timeline, as text (tools/lk_timeline.py reads it)
        const uint32_t nwg = std::min<uint32_t>(sg, kTlMaxWg), nt = (uint32_t)std::min<uint64_t>(stiles, kTlMaxTiles);
        std::vector<unsigned long long> wg(2 * kTlMaxWg), te(kTlMaxTiles);
        std::vector<uint32_t> hw(2 * kTlMaxWg), tw(kTlMaxTiles);
        RP_HIP(hipStreamSynchronize(st));
        RP_HIP(hipMemcpyFromSymbol(wg.data(), HIP_SYMBOL(g_tl_wg), 8 * wg.size()));
        RP_HIP(hipMemcpyFromSymbol(hw.data(), HIP_SYMBOL(g_tl_hw), 4 * hw.size()));
        RP_HIP(hipMemcpyFromSymbol(te.data(), HIP_SYMBOL(g_tl_tile), 8 * te.size()));
        RP_HIP(hipMemcpyFromSymbol(tw.data(), HIP_SYMBOL(g_tl_tile_wg), 4 * tw.size()));
        if (FILE* f = fopen(k.tl_dump, "w")) {
            fprintf(f, "# sort %d ticket %d grid %u stagger %d tiles %llu\n", sort_t, ticket ? 1 : 0, sg, stag16,
                    (unsigned long long)stiles);
            for (uint32_t i = 0; i < nwg; i++)
                fprintf(f, "W %u %u %u %llu %llu\n", i, hw[2 * i], hw[2 * i + 1], wg[2 * i], wg[2 * i + 1]);
            for (uint32_t i = 0; i < nt; i++) fprintf(f, "T %u %u %llu\n", i, tw[i], te[i]);
            fclose(f);
        }
    }
#endif
    // (t0 > 0: TK is 2048, the lists are uniform)
    lookupn_tiles_end(r, k, b, t0 + ntiles, TK, done, cv.ablate != 3 && !fuse, 0,
                      [&](auto keys_done, auto tot, auto over, const uint32_t*) {
                          fprintf(stderr, "[rp] compact lookupN: %llu keys, %llu deferred, %llu overflowed tiles (cb %u ob %u fsh %u sort %d) "
                                          "ticket %d grid %u stagger %d\n",
                                  keys_done, tot, over, r.ccb, r.cob, r.cfsh, sort_t, ticket ? 1 : 0, sg, stag16);
                      });
}

// The packed layout's window probe, its deferred keys finished by k_lookupn_fix
static bool lookupn_probe(Ring& r, const LookupKnobs& k, const Batch36& b) {
    if (b.W > 4 || b.need > 4 || k.nowindow) return false;
    RP_REQUIRE(b.n < (1ull << 32), "lookupn: at most 2^32-1 keys per call");
    r.slow.reserve(b.n + 1);
    r.nslow.reserve(1);
    RP_HIP(hipMemsetAsync(r.nslow.p, 0, sizeof(uint32_t), b.st));
    const int kpl = k.kpl_set ? k.kpl : kDefaultKPL;
    const PackedView pv = r.pview();
    const auto probe = [&](auto keys_per_lane, auto mode) {
        constexpr int KPL = decltype(keys_per_lane)::value, MODE = decltype(mode)::value;
        hipLaunchKernelGGL((k_lookupn_probe<36, KPL, MODE>), dim3(grid_for(b.n, kLkThreads * KPL, 256 * 8)),
                           dim3(kLkThreads), 0, b.st, b.keys, b.n, pv, b.np, b.W, b.out, b.counts, r.slow.p, r.nslow.p);
        hipLaunchKernelGGL((k_lookupn_fix<36, MODE>), dim3(256), dim3(256), 0, b.st, b.keys, pv, b.np, b.W, b.out,
                           b.counts, r.slow.p, r.nslow.p);
    };
    if (k.ablate == 1)
        probe(Int<2>{}, Int<1>{});
    else if (k.ablate == 2)
        probe(Int<2>{}, Int<2>{});
    else if (kpl == 1)
        probe(Int<1>{}, Int<0>{});
    else if (kpl == 4)
        probe(Int<4>{}, Int<0>{});
    else if (kpl == 8)
        probe(Int<8>{}, Int<0>{});
    else
        probe(Int<2>{}, Int<0>{});
    RP_HIP(hipGetLastError());
    return true;
}

static void launch_lookupn(Ring& r, const uint8_t* keys, const uint64_t* off, uint32_t stride,
                           const uint32_t* hashes, uint64_t n, int np, uint32_t W, uint32_t* out, uint8_t* counts,
                           hipStream_t st) {
    if (n == 0) return;
    // the ring is rebuilt on r.st; make the caller's stream wait for it
    if (st != r.st) RP_HIP(hipStreamSynchronize(r.st));
    const LookupKnobs k = lookup_knobs();
    const bool fixed36 = DevKeys{keys, off, stride, hashes}.fixed36();
    const int need = np <= 0 ? 1 : np;
    const bool use_packed = r.packed && !k.wide;
    const bool use_compact = r.compact && !k.layout_packed && !k.wide;
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(keys) & 15) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
    const Batch36 b{keys, n, np, need, W, out, counts, st};  // (read only where fixed36)
    // whole tiles of keys through 16-byte loads, whole rows of `need` owners through 16-byte stores
    const bool tiled = use_compact && fixed36 && aligned16 && (uint32_t)need == W && W <= 4;
    if (tiled && lookupn_lds(r, k, b)) return;
    if (tiled && n >= (uint64_t)kLkThreads * 4) {
        RP_REQUIRE(n < (1ull << 32), "lookupn: at most 2^32-1 keys per call");
        if (r.chint_pending && need == 3) ring_build_hint(r);
        const CompactView cv = r.cview(k);
        if (!lookupn_ws(r, k, b, cv)) lookupn_compact(r, k, b, cv);
        return;
    }
    if (use_packed && fixed36 && lookupn_probe(r, k, b)) return;
    if (use_packed)
        launch_lookupn_view(r.pview(), keys, off, stride, hashes, n, np, W, out, counts, st, k.ablate);
    else
        launch_lookupn_view(r.view(), keys, off, stride, hashes, n, np, W, out, counts, st, k.ablate);
}

// ------------------------------------------------------------------- group keys by owner
// RingPop.handleOrProxyAll's keysByDest = _.groupBy(keys, this.lookup) (index.js:609-667, :616)
// and RequestProxySend.lookupKeys (lib/request-proxy/send.js:171-179). _.groupBy appends each
// key to its owner's list in input order and Object.keys(keysByDest) lists the owners in
// first-seen order, so: first[s] = min key index owned by s; the owners ranked by first[s];
// a stable sort of the key indices by that rank.

__global__ void k_grp_first(const uint32_t* __restrict__ own, uint64_t n, uint32_t* __restrict__ first) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gstride) {
        const uint32_t s = own[i];
        // a plain (possibly stale) read first: once an owner's first key is known, later keys
        // skip the atomic
        if ((uint32_t)i < first[s]) atomicMin(first + s, (uint32_t)i);
    }
}

// (first index, owner) pairs to sort; unseen owners sort after every seen one (key n)
__global__ void k_grp_dest_keys(const uint32_t* __restrict__ first, uint32_t S, uint32_t n,
                                uint32_t* __restrict__ dk, uint32_t* __restrict__ dv) {
    const uint32_t gstride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < S; s += gstride) {
        const uint32_t f = first[s];
        dk[s] = f < n ? f : n;
        dv[s] = s;
    }
}

// owners in first-seen order: dests[p], rank[owner] = p, *ndest
__global__ void k_grp_rank(const uint32_t* __restrict__ dk, const uint32_t* __restrict__ dv, uint32_t S, uint32_t n,
                           uint32_t* __restrict__ rank, uint32_t* __restrict__ dests, uint32_t* __restrict__ ndest) {
    const uint32_t gstride = gridDim.x * blockDim.x;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < S; p += gstride) {
        if (dk[p] >= n) continue;
        rank[dv[p]] = p;
        dests[p] = dv[p];
        if (p + 1 == S || dk[p + 1] >= n) *ndest = p + 1;
    }
}

// sort keys: the owner's rank; values: the key index (stable sort keeps input order per group)
__global__ void k_grp_keys(const uint32_t* __restrict__ own, uint64_t n, const uint32_t* __restrict__ rank,
                           uint32_t* __restrict__ gk, uint32_t* __restrict__ perm) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gstride) {
        gk[i] = rank[own[i]];
        perm[i] = (uint32_t)i;
    }
}

// group_off[g] = first position of rank g in the sorted keys; group_off[ndest] = n
__global__ void k_grp_bounds(const uint32_t* __restrict__ gk, uint64_t n, uint32_t* __restrict__ goff) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gstride) {
        const uint32_t g = gk[p];
        if (p == 0 || gk[p - 1] != g) goff[g] = (uint32_t)p;
        if (p + 1 == n) goff[g + 1] = (uint32_t)n;
    }
}

static int bits_for(uint64_t v) {  // radix bits (multiple of 8) that hold every value <= v
    int b = 8;
    while (b < 32 && (v >> b)) b += 8;
    return b;
}

// keys (or caller hashes) -> owners -> groups; buffers as rp_ring_group_keys_dev documents
static void group_keys(Ring& r, const uint8_t* keys, const uint64_t* off, uint32_t stride, const uint32_t* hashes,
                       uint64_t n, uint32_t self_id, uint32_t* dests, uint32_t* goff, uint32_t* perm,
                       uint32_t* ndest, hipStream_t st) {
    RP_REQUIRE(n < 0xFFFFFFFFull, "group_keys: at most 2^32-2 keys per call");
    if (st != r.st) RP_HIP(hipStreamSynchronize(r.st));
    if (n == 0 || r.M == 0) {
        // lookup returns null for every key and RingPop.lookup answers whoami() (index.js:434-451):
        // one group (self) holding every key in order, or no group at all
        const uint32_t h[3] = {self_id, 0u, (uint32_t)n};
        const uint32_t nd = n ? 1u : 0u;
        RP_HIP(hipMemcpyAsync(ndest, &nd, 4, hipMemcpyHostToDevice, st));
        if (n) {
            RP_HIP(hipMemcpyAsync(dests, h, 4, hipMemcpyHostToDevice, st));
            RP_HIP(hipMemcpyAsync(goff, h + 1, 8, hipMemcpyHostToDevice, st));
            iota_u32(perm, n, st);
        } else {
            RP_HIP(hipMemsetAsync(goff, 0, 4, st));
        }
        RP_HIP(hipStreamSynchronize(st));  // h lives on this stack frame
        return;
    }
    const uint32_t S = r.nt.size();
    r.grp_own.reserve(n);
    r.grp_key.reserve(n);
    r.grp_first.reserve(S);
    r.grp_dk.reserve(S);
    r.grp_dv.reserve(S);
    r.grp_rank.reserve(S);
    launch_lookupn(r, keys, off, stride, hashes, n, 1, 1, r.grp_own.p, nullptr, st);
    RP_HIP(hipMemsetAsync(r.grp_first.p, 0xFF, 4ull * S, st));
    hipLaunchKernelGGL(k_grp_first, dim3(grid_for(n, 256, 256 * 16)), dim3(256), 0, st, r.grp_own.p, n, r.grp_first.p);
    hipLaunchKernelGGL(k_grp_dest_keys, dim3(grid_for(S, 256)), dim3(256), 0, st, r.grp_first.p, S, (uint32_t)n,
                       r.grp_dk.p, r.grp_dv.p);
    radix_sort_pairs(r.grp_dk.p, r.grp_dv.p, S, 0, bits_for(n), st, r.ws);
    hipLaunchKernelGGL(k_grp_rank, dim3(grid_for(S, 256)), dim3(256), 0, st, r.grp_dk.p, r.grp_dv.p, S, (uint32_t)n,
                       r.grp_rank.p, dests, ndest);
    hipLaunchKernelGGL(k_grp_keys, dim3(grid_for(n, 256, 256 * 16)), dim3(256), 0, st, r.grp_own.p, n, r.grp_rank.p,
                       r.grp_key.p, perm);
    radix_sort_pairs(r.grp_key.p, perm, n, 0, bits_for(S - 1), st, r.ws);
    hipLaunchKernelGGL(k_grp_bounds, dim3(grid_for(n, 256, 256 * 16)), dim3(256), 0, st, r.grp_key.p, n, goff);
    RP_HIP(hipGetLastError());
}

// ------------------------------------------------------------- ring snapshots and moved keys
// A snapshot is a device copy of the exact wide arrays (RingView) with the counts and checksum of
// its moment. k_moved diffs two rings over one key stream: each key is read and hashed once, both
// rings are searched and walked from that hash on their exact views (moved_find / moved_walk; no
// fingerprints, so no key is ever deferred), the two rows are compared in registers, and only the moved keys leave the
// kernel. Order-preserving compaction in one launch: wave ballots + popcounts, per-workgroup
// totals in LDS, and the tile's global offset by decoupled look-back (tile = ticket, so tiles are
// in key order and every tile a tile waits on is already running).
struct Snap {
    int device = 0;
    DevBuf<uint32_t> tok, own, bstart;
    uint32_t M = 0, bbits = 8, server_count = 0, checksum = 0;
    uint32_t id_bound = 0;  // the ring's interned ids at snapshot time (the owner-load id_cap check)
    bool has_checksum = false;
    LoadScratch load_ws;  // owner load / share (allocated at first use)
    RangeScratch range_ws;  // moved ranges, when this snapshot is the `after` side (allocated at first use)
    RingView view() const { return RingView{tok.p, own.p, bstart.p, M, 32u - bbits}; }
};

// Exact search and walk on the wide arrays with one load instruction per step, as the lean kernel
// does on the compact layout (every lane of a load instruction that touches another line is one
// L1->L2 request, and the lookups are bound by those): the bucket's [lo, hi) as one 8-B load, its
// tokens four at a time as one 16-B load (buckets hold ~4 tokens), the successor owners four at a
// time as one 16-B load. Every load stays inside [0, M); windows that would cross M fall back to
// single loads. Results equal RingView::find + ring_walk exactly.
__device__ __forceinline__ uint32_t moved_find(const RingView& rv, uint32_t h) {
    const uint32_t b = h >> rv.shift;
    const u32x2_a4 be = *reinterpret_cast<const u32x2_a4*>(rv.bstart + b);
    uint32_t lo = be.x, hi = be.y;
    if (hi - lo > 16) {  // a crowded bucket (caller hashFunc values that collide): binary search
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (rv.tok[mid] < h) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
    while (lo < hi) {
        const uint32_t n = hi - lo < 4u ? hi - lo : 4u;
        uint32_t c;
        if (lo + 4u <= rv.M) {
            const u32x4_a4 t = *reinterpret_cast<const u32x4_a4*>(rv.tok + lo);
            c = (uint32_t)(t.x < h) + (uint32_t)((n > 1u) & (t.y < h)) + (uint32_t)((n > 2u) & (t.z < h)) +
                (uint32_t)((n > 3u) & (t.w < h));  // (sorted: the tokens below h are a prefix)
        } else {
            c = 0;
            while (c < n && rv.tok[lo + c] < h) c++;
        }
        lo += c;
        if (c < 4u) break;
    }
    return lo;
}

template <int MAXN>
__device__ __forceinline__ void moved_walk(const RingView& rv, uint32_t i, int np, uint32_t (&res)[MAXN]) {
#pragma unroll
    for (int q = 0; q < MAXN; q++) res[q] = NIL;
    if (rv.M == 0) return;
    if (np <= 0) {
        if (i < rv.M) res[0] = rv.own[i];
        return;
    }
    uint32_t j = (i == rv.M) ? 0u : i;
    if (MAXN == 1) {
        res[0] = rv.own[j];
        return;
    }
    int cnt = 0;
    auto take = [&](uint32_t o) {
        bool dup = false;
#pragma unroll
        for (int q = 0; q < MAXN; q++) dup |= (q < cnt) & (res[q] == o);
        if (!dup) {
#pragma unroll
            for (int q = 0; q < MAXN; q++) res[q] = (q == cnt) ? o : res[q];
            cnt++;
        }
    };
    uint32_t steps = 0;
    while (steps < rv.M && cnt < np) {
        if (j + 4u <= rv.M) {
            const u32x4_a4 o = *reinterpret_cast<const u32x4_a4*>(rv.own + j);
            const uint32_t o4[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (steps < rv.M && cnt < np) {
                    take(o4[k]);
                    steps++;
                }
            j = (j + 4u == rv.M) ? 0u : j + 4u;
        } else {
            take(rv.own[j]);
            steps++;
            j = (j + 1u == rv.M) ? 0u : j + 1u;
        }
    }
}

// The tile passes' shared pieces (k_moved, k_handoff). One tile of TILE = 256 * KPL keys per
// workgroup, tile = ticket.
//
// stage_tile36: the tile's `cnt` 36-byte keys from keys + base * 36 (a 4-byte aligned base) into
// sk[TILE * 9]: full tiles of a 16-byte aligned base with non-temporal 16-B loads (read once; they
// must not evict the two rings' tables from L2), every other tile dword by dword. Syncs.
template <int TILE>
__device__ __forceinline__ void stage_tile36(uint32_t* sk, const uint8_t* __restrict__ keys, uint32_t base,
                                             uint32_t cnt, int tid) {
    constexpr int W4 = 9;                    // dwords per 36-byte key
    constexpr int V4 = TILE * W4 / 4;        // 16-B vectors per full tile
    constexpr int PER = (V4 + kLkThreads - 1) / kLkThreads;
    static_assert((TILE * W4) % 4 == 0, "tile must be a whole number of 16-B vectors");
    const uint8_t* src = keys + (uint64_t)base * 36u;
    if (cnt == (uint32_t)TILE && (reinterpret_cast<uintptr_t>(keys) & 15) == 0) {
        const u32x4* s4 = reinterpret_cast<const u32x4*>(src);
        u32x4* d4 = reinterpret_cast<u32x4*>(sk);
        u32x4 pre[PER];
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int k = tid + q * kLkThreads;
            if (k < V4) pre[q] = __builtin_nontemporal_load(s4 + k);
        }
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int k = tid + q * kLkThreads;
            if (k < V4) d4[k] = pre[q];
        }
    } else {
        const uint32_t* s1 = reinterpret_cast<const uint32_t*>(src);
        for (uint32_t k = tid; k < cnt * W4; k += kLkThreads) sk[k] = s1[k];
    }
    __syncthreads();
}

// tile_offset: the order-preserving compaction's tail. Every wave's lane 0 has stored its record
// count of slot q in s_cnt[q * 4 + wave]; this gives pre[q], the records of the tile before the
// caller's (slot q, wave) segment, publishes the tile's total, returns the records of all earlier
// tiles (decoupled look-back) and has the last tile write *count. Syncs before and after.
template <int KPL>
__device__ __forceinline__ uint32_t tile_offset(const uint32_t* s_cnt, uint32_t* s_excl, uint64_t* __restrict__ lb,
                                                uint32_t tile, uint64_t tag, uint32_t ntiles,
                                                uint32_t* __restrict__ count, uint32_t* err, uint32_t (&pre)[KPL]) {
    const int tid = threadIdx.x, wave = tid >> 6;
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int s = 0; s < KPL * (kLkThreads / 64); s++) {
        if ((s & (kLkThreads / 64 - 1)) == wave) pre[s / (kLkThreads / 64)] = total;
        total += s_cnt[s];
    }
    if (tid == 0) lb_store(lb + tile, tag | (tile == 0 ? kLbP : kLbA) | total);
    if (tid < 64) {
        const uint32_t excl = lookback_wave(lb, tile, tag, err);
        if (tid == 0) {
            if (tile > 0) lb_store(lb + tile, tag | kLbP | (excl + total));
            *s_excl = excl;
            if (tile == ntiles - 1) *count = excl + total;
        }
    }
    __syncthreads();
    return *s_excl;
}

// FIXED: 36-byte keys at stride 36 from a 4-byte aligned base, staged through LDS (stage_tile36).
// Otherwise: per-thread byte fetches (offsets, any stride, any base) or precomputed hashes
// (key_hash). Key q * 256 + tid of the tile in slot q of thread tid, so that (q, wave, lane) order
// is key order.
template <int MAXN, int KPL, bool FIXED>
__global__ __launch_bounds__(kLkThreads) void k_moved(const uint8_t* __restrict__ keys,
                                                      const uint64_t* __restrict__ off, uint32_t stride,
                                                      const uint32_t* __restrict__ hashes, uint32_t n, RingView bv,
                                                      int npb, RingView av, int npa, uint32_t W, uint32_t cap,
                                                      uint32_t* __restrict__ idx, uint32_t* __restrict__ brow,
                                                      uint32_t* __restrict__ arow, uint32_t* __restrict__ count,
                                                      uint64_t* __restrict__ lb, unsigned long long* ctr,
                                                      uint64_t tag, uint32_t ntiles, uint32_t* err) {
    constexpr int TILE = kLkThreads * KPL;
    __shared__ __attribute__((aligned(16))) uint32_t sk[FIXED ? TILE * 9 : 4];
    __shared__ uint32_t s_cnt[KPL * (kLkThreads / 64)];
    __shared__ uint32_t s_excl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile = take_unit(ctr, ntiles, err);  // (syncs)
    if (tile >= ntiles) return;  // a ticket count out of step (reported): never write out of bounds
    const uint32_t base = tile * (uint32_t)TILE;
    const uint32_t cnt = n - base < (uint32_t)TILE ? n - base : (uint32_t)TILE;
    if constexpr (FIXED) stage_tile36<TILE>(sk, keys, base, cnt, tid);
    uint32_t rb[KPL][MAXN], ra[KPL][MAXN];
    bool mv[KPL];
#pragma unroll
    for (int q = 0; q < KPL; q++) {
        const uint32_t kl = (uint32_t)(q * kLkThreads + tid);
        mv[q] = false;
#pragma unroll
        for (int j = 0; j < MAXN; j++) rb[q][j] = ra[q][j] = NIL;
        if (kl < cnt) {
            const uint32_t h = FIXED ? key_hash36(sk + kl * 9) : key_hash(keys, off, stride, hashes, (uint64_t)base + kl);
            moved_walk<MAXN>(bv, moved_find(bv, h), npb, rb[q]);
            moved_walk<MAXN>(av, moved_find(av, h), npa, ra[q]);
            bool d = false;
#pragma unroll
            for (int j = 0; j < MAXN; j++) d |= rb[q][j] != ra[q][j];
            mv[q] = d;
        }
    }
    // ranks inside the wave's 64 keys of slot q, and the (slot, wave) segment totals
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t rank[KPL];
#pragma unroll
    for (int q = 0; q < KPL; q++) {
        const uint64_t m = __ballot(mv[q]);
        rank[q] = (uint32_t)__popcll(m & lt_mask);
        if (lane == 0) s_cnt[q * (kLkThreads / 64) + wave] = (uint32_t)__popcll(m);
    }
    uint32_t pre[KPL];
    const uint32_t gbase = tile_offset<KPL>(s_cnt, &s_excl, lb, tile, tag, ntiles, count, err, pre);
#pragma unroll
    for (int q = 0; q < KPL; q++) {
        const uint32_t p = gbase + pre[q] + rank[q];
        if (mv[q] && p < cap) {  // (also bounds every write if a look-back wait gave up)
            idx[p] = base + (uint32_t)(q * kLkThreads + tid);
#pragma unroll
            for (int j = 0; j < MAXN; j++) {
                if ((uint32_t)j < W) {
                    if (brow) brow[(uint64_t)p * W + j] = rb[q][j];
                    if (arow) arow[(uint64_t)p * W + j] = ra[q][j];
                }
            }
        }
    }
}

// A tile pass over n keys: one workgroup a tile of 256 * KPL keys, the look-back state after `args`
template <int KPL, class Kernel, class... A>
static void launch_tiles(Kernel kernel, uint32_t n, hipStream_t st, Scratch& ws, A... args) {
    const uint32_t ntiles = (uint32_t)(((uint64_t)n + kLkThreads * KPL - 1) / (kLkThreads * KPL));
    const LookBack L = lookback_prepare(ws, ntiles, st);
    hipLaunchKernelGGL(kernel, dim3(ntiles), dim3(kLkThreads), 0, st, args..., L.words, L.ticket, L.tag, ntiles, L.err);
    RP_HIP(hipGetLastError());
}

// f(Int<MAXN>{}, Int<KPL>{}, FIXED{}): the tile passes' kernel shape for rows of W slots. Staged
// 36-byte keys go four a lane (two with rows of eight), every other form one.
template <class F>
static void with_tile_shape(uint32_t W, bool fixed36, F&& f) {
    if (fixed36) {
        if (W == 1) f(Int<1>{}, Int<4>{}, std::true_type{});
        else if (W <= 4) f(Int<4>{}, Int<4>{}, std::true_type{});
        else f(Int<8>{}, Int<2>{}, std::true_type{});
    } else {
        if (W == 1) f(Int<1>{}, Int<1>{}, std::false_type{});
        else if (W <= 4) f(Int<4>{}, Int<1>{}, std::false_type{});
        else f(Int<8>{}, Int<1>{}, std::false_type{});
    }
}

// before / after rows of W slots each; outputs as rp_ring_moved_keys_dev documents
static void moved_keys(Ring& r, const Snap& s, const DevKeys& k, uint64_t n, int32_t nrep, uint32_t cap, uint32_t* idx,
                       uint32_t* brow, uint32_t* arow, uint32_t* count, hipStream_t st) {
    RP_REQUIRE(nrep <= 8, "moved_keys: nrep is at most 8 (the rows are compared in registers)");
    RP_REQUIRE(n < (1ull << 32), "moved_keys: at most 2^32-1 keys per call");
    RP_REQUIRE(s.device == r.device, "moved_keys: the snapshot lives on another device");
    RP_REQUIRE(count, "moved_keys: null count");
    RP_REQUIRE(cap == 0 || idx, "moved_keys: null index buffer");
    // the ring is rebuilt on r.st; make the caller's stream wait for it
    if (st != r.st) RP_HIP(hipStreamSynchronize(r.st));
    if (n == 0 || (r.M == 0 && s.M == 0)) {
        RP_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), st));
        return;
    }
    const int npb = replicas(nrep, s.server_count).np;
    const auto [npa, W] = replicas(nrep, r.server_count);
    const RingView bv = s.view(), av = r.view();
    with_tile_shape(W, k.fixed36(), [&, npa = npa, W = W](auto maxn, auto kpl, auto fixed) {
        launch_tiles<kpl()>(k_moved<maxn(), kpl(), fixed()>, (uint32_t)n, st, r.ws, k.keys, k.off, k.stride, k.hashes,
                            (uint32_t)n, bv, npb, av, npa, W, cap, idx, brow, arow, count);
    });
}

// ------------------------------------------------------------- hand-off plan
// What to send to whom after a ring change (rp_ring_handoff*). k_handoff is k_moved's pass with
// another tail: per key the two rows (moved_find / moved_walk, the same tile = ticket scheme and
// key staging), then in registers the gained mask (each entry of the row now against the whole
// row before) and, for keys that gain a server only, the source: the first holder before that is
// in the ring now (one byte of d_inring per holder until one is live). A key emits one record per
// gained server, so the compaction is multi-record: a key's first record has rank
// sum_j popcount(ballot(c > j) & lanes below) among its wave's keys of a slot, c its record
// count; (slot, wave) prefixes in LDS; the tile's offset by decoupled look-back. The record
// stream (key index, dst, src, slot) goes to the ring's scratch in (key, slot) order below cap;
// a stable sort by dst then groups it.
template <int MAXN, int KPL, bool FIXED>
__global__ __launch_bounds__(kLkThreads) void k_handoff(const uint8_t* __restrict__ keys,
                                                        const uint64_t* __restrict__ off, uint32_t stride,
                                                        const uint32_t* __restrict__ hashes, uint32_t n, RingView bv,
                                                        int npb, RingView av, int npa,
                                                        const uint8_t* __restrict__ inring, uint32_t ninring,
                                                        uint32_t only_src, uint32_t cap, uint32_t* __restrict__ rkey,
                                                        uint32_t* __restrict__ rdst, uint32_t* __restrict__ rsrc,
                                                        uint8_t* __restrict__ rslot, uint32_t* __restrict__ count,
                                                        uint64_t* __restrict__ lb, unsigned long long* ctr,
                                                        uint64_t tag, uint32_t ntiles, uint32_t* err) {
    constexpr int TILE = kLkThreads * KPL;
    __shared__ __attribute__((aligned(16))) uint32_t sk[FIXED ? TILE * 9 : 4];
    __shared__ uint32_t s_cnt[KPL * (kLkThreads / 64)];
    __shared__ uint32_t s_excl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile = take_unit(ctr, ntiles, err);  // (syncs)
    if (tile >= ntiles) return;  // a ticket count out of step (reported): never write out of bounds
    const uint32_t base = tile * (uint32_t)TILE;
    const uint32_t cnt = n - base < (uint32_t)TILE ? n - base : (uint32_t)TILE;
    if constexpr (FIXED) stage_tile36<TILE>(sk, keys, base, cnt, tid);
    uint32_t ra[KPL][MAXN], gm[KPL], sr[KPL];  // the row now, its gained slots (bit q), the source
#pragma unroll
    for (int q = 0; q < KPL; q++) {
        const uint32_t kl = (uint32_t)(q * kLkThreads + tid);
        gm[q] = 0;
        sr[q] = NIL;
#pragma unroll
        for (int j = 0; j < MAXN; j++) ra[q][j] = NIL;
        if (kl < cnt) {
            const uint32_t h = FIXED ? key_hash36(sk + kl * 9) : key_hash(keys, off, stride, hashes, (uint64_t)base + kl);
            uint32_t rb[MAXN];
            moved_walk<MAXN>(bv, moved_find(bv, h), npb, rb);
            moved_walk<MAXN>(av, moved_find(av, h), npa, ra[q]);
            uint32_t g = 0;
#pragma unroll
            for (int a = 0; a < MAXN; a++) {
                bool held = false;
#pragma unroll
                for (int b = 0; b < MAXN; b++) held |= ra[q][a] == rb[b];
                if (ra[q][a] != NIL && !held) g |= 1u << a;
            }
            if (g) {
                uint32_t s = NIL;
#pragma unroll
                for (int b = 0; b < MAXN; b++)
                    if (s == NIL && rb[b] < ninring && inring[rb[b]]) s = rb[b];  // (NIL >= ninring)
                sr[q] = s;
                if (only_src != NIL && s != only_src) g = 0;
            }
            gm[q] = g;
        }
    }
    // a key's first record among the records of its wave's 64 keys of slot q, and the
    // (slot, wave) segment totals
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t rank[KPL];
#pragma unroll
    for (int q = 0; q < KPL; q++) {
        const int c = __popc(gm[q]);
        uint32_t rk = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < MAXN; j++) {
            const uint64_t m = __ballot(c > j);
            rk += (uint32_t)__popcll(m & lt_mask);
            tot += (uint32_t)__popcll(m);
        }
        rank[q] = rk;
        if (lane == 0) s_cnt[q * (kLkThreads / 64) + wave] = tot;
    }
    uint32_t pre[KPL];
    const uint32_t gbase = tile_offset<KPL>(s_cnt, &s_excl, lb, tile, tag, ntiles, count, err, pre);
#pragma unroll
    for (int q = 0; q < KPL; q++) {
        uint32_t p = gbase + pre[q] + rank[q];
#pragma unroll
        for (int j = 0; j < MAXN; j++) {
            if ((gm[q] >> j) & 1u) {
                if (p < cap) {  // (also bounds every write if a look-back wait gave up)
                    rkey[p] = base + (uint32_t)(q * kLkThreads + tid);
                    rdst[p] = ra[q][j];
                    rsrc[p] = sr[q];
                    rslot[p] = (uint8_t)j;
                }
                p++;
            }
        }
    }
}

// Grouping: the records sorted by dst (stable, so (key, slot) order inside a group). T =
// min(*count, cap) is read on the device; threads past T exit.
// present[d] = 1 for every dst among the first T sorted records (the run heads)
__global__ void k_handoff_heads(const uint32_t* __restrict__ sd, const uint32_t* __restrict__ count, uint32_t cap,
                                uint32_t id_bound, uint32_t* __restrict__ present) {
    const uint32_t T = *count < cap ? *count : cap;
    const uint32_t gstride = gridDim.x * blockDim.x;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < T; p += gstride) {
        const uint32_t d = sd[p];
        if ((p == 0 || sd[p - 1] != d) && d < id_bound) present[d] = 1u;
    }
}

// rank = the exclusive scan of present (rank[id_bound] = the number of destinations): dests and
// group_off from the run heads, and the record columns gathered through the sort's permutation
__global__ void k_handoff_emit(const uint32_t* __restrict__ sd, const uint32_t* __restrict__ perm,
                               const uint32_t* __restrict__ rkey, const uint32_t* __restrict__ rsrc,
                               const uint8_t* __restrict__ rslot, const uint32_t* __restrict__ count, uint32_t cap,
                               uint32_t id_bound, const uint32_t* __restrict__ rank, uint32_t* __restrict__ dests,
                               uint32_t* __restrict__ goff, uint32_t* __restrict__ key_idx,
                               uint32_t* __restrict__ src, uint8_t* __restrict__ slot, uint32_t* __restrict__ ndest) {
    const uint32_t T = *count < cap ? *count : cap;
    const uint32_t gstride = gridDim.x * blockDim.x;
    const uint32_t t0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 == 0) {
        *ndest = T ? rank[id_bound] : 0u;
        if (T == 0 && goff) goff[0] = 0u;
    }
    for (uint32_t p = t0; p < T; p += gstride) {
        const uint32_t d = sd[p], i = perm[p];
        key_idx[p] = rkey[i];
        if (src) src[p] = rsrc[i];
        if (slot) slot[p] = rslot[i];
        if (d >= id_bound) continue;  // (no row holds such an id)
        const uint32_t g = rank[d];
        if (p == 0 || sd[p - 1] != d) {
            dests[g] = d;
            goff[g] = p;
        }
        if (p + 1 == T) goff[g + 1] = T;
    }
}

// The plan between the snapshot s and the ring now; device outputs as rp_ring_handoff_dev
// documents. known_count: the host forms read the record count back after the first pass and
// group exactly min(count, cap) records; the device form groups over min(cap, n * W) slots,
// padded with a key that sorts last.
static void handoff(Ring& r, const Snap& s, const DevKeys& k, uint64_t n, int32_t nrep, uint32_t only_src,
                    uint32_t cap, uint32_t* dests, uint32_t* goff, uint32_t* key_idx, uint32_t* src, uint8_t* slot,
                    uint32_t* ndest, uint32_t* count, hipStream_t st, bool known_count) {
    const int npb = replicas(nrep, s.server_count).np;
    const auto [npa, W] = replicas(nrep, r.server_count);
    const uint32_t id_bound = r.nt.size();
    RP_REQUIRE(nrep <= 8, "handoff: nrep is at most 8 (the rows are compared in registers)");
    RP_REQUIRE(n < (1ull << 32) && n * W < (1ull << 32), "handoff: n * max(nrep, 1) is at most 2^32-1 records");
    RP_REQUIRE(s.device == r.device, "handoff: the snapshot lives on another device");
    RP_REQUIRE(only_src == NIL || only_src < id_bound, "handoff: only_src is not a server id of this ring");
    RP_REQUIRE(ndest && count, "handoff: null count");
    RP_REQUIRE(cap == 0 || (dests && goff && key_idx), "handoff: null output buffer");
    // the ring is rebuilt on r.st; make the caller's stream wait for it
    if (st != r.st) RP_HIP(hipStreamSynchronize(r.st));
    if (n == 0 || r.M == 0) {  // no key, or nothing to gain
        RP_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), st));
        RP_HIP(hipMemsetAsync(ndest, 0, sizeof(uint32_t), st));
        if (goff) RP_HIP(hipMemsetAsync(goff, 0, sizeof(uint32_t), st));
        return;
    }
    HandoffScratch& ws = r.handoff_ws;
    ws.use_on(st);
    const uint32_t m = (uint32_t)std::min<uint64_t>(cap, n * W);  // record slots
    ws.key.reserve(m);
    ws.dst.reserve(m);
    ws.src.reserve(m);
    ws.slot.reserve(m);
    ws.perm.reserve(m);
    ws.rank.reserve((uint64_t)id_bound + 1);
    const int sort_bits = bits_for(id_bound);
    // the slots past the record count sort last (0xFF..: above every id in the sorted bits)
    if (m && !known_count) RP_HIP(hipMemsetAsync(ws.dst.p, 0xFF, 4ull * m, st));
    const RingView bv = s.view(), av = r.view();
    with_tile_shape(W, k.fixed36(), [&, npa = npa](auto maxn, auto kpl, auto fixed) {
        launch_tiles<kpl()>(k_handoff<maxn(), kpl(), fixed()>, (uint32_t)n, st, r.ws, k.keys, k.off, k.stride, k.hashes,
                            (uint32_t)n, bv, npb, av, npa, (const uint8_t*)r.d_inring.p, r.inring_n, only_src, m,
                            ws.key.p, ws.dst.p, ws.src.p, ws.slot.p, count);
    });
    if (m == 0) {  // counts only
        RP_HIP(hipMemsetAsync(ndest, 0, sizeof(uint32_t), st));
        if (goff) RP_HIP(hipMemsetAsync(goff, 0, sizeof(uint32_t), st));
        return;
    }
    uint32_t g = m;  // the slots to group
    if (known_count) {
        uint32_t total = 0;
        RP_HIP(hipMemcpyAsync(&total, count, 4, hipMemcpyDeviceToHost, st));
        RP_HIP(hipStreamSynchronize(st));
        scratch_check(r.ws, st);  // a look-back wait that gave up is an error, not a wrong plan
        g = std::min(total, m);
    }
    if (g) {
        iota_u32(ws.perm.p, g, st);
        radix_sort_pairs(ws.dst.p, ws.perm.p, g, 0, sort_bits, st, r.ws);
    }
    RP_HIP(hipMemsetAsync(ws.rank.p, 0, 4ull * ((uint64_t)id_bound + 1), st));
    hipLaunchKernelGGL(k_handoff_heads, dim3(grid_for(g, 256, 256 * 16)), dim3(256), 0, st, ws.dst.p, count, g,
                       id_bound, ws.rank.p);
    RP_HIP(hipGetLastError());
    scan_exclusive_u32(ws.rank.p, ws.rank.p, id_bound, st, r.ws);
    hipLaunchKernelGGL(k_handoff_emit, dim3(grid_for(g, 256, 256 * 16)), dim3(256), 0, st, ws.dst.p, ws.perm.p,
                       ws.key.p, ws.src.p, ws.slot.p, count, g, id_bound, ws.rank.p, dests, goff, key_idx, src, slot,
                       ndest);
    RP_HIP(hipGetLastError());
}

// ------------------------------------------------------------- owner load and hash-space share
// load[id * W + q] = how many keys have server `id` in slot q of their lookupN row. The lookup
// kernels are not forked: the key stream is walked in chunks, launch_lookupn / launch_lookupn_view
// writes a chunk's rows into a handle-owned scratch (16-B aligned: the lean path), and k_owner_load
// counts those rows on the same stream, so the rows are what rp_ring_lookupn* writes on every
// layout, key form and nrep, and the extra memory is chunk * W * 4 bytes whatever n is.
constexpr int kLoadThreads = 1024;
constexpr uint32_t kLoadBins = 32768;         // uint32 LDS bins of one launch's window (128 KB of gfx950's 160 KB)
constexpr uint32_t kLoadBins2 = 20480;        // at most this many LDS words: two workgroups share a CU (80 KB each)
constexpr uint64_t kLoadChunk = 1ull << 24;   // keys a chunk (RP_LOAD_CHUNK): the best of the 2^20..2^24 sweep, DESIGN 4.2c
constexpr uint64_t kLoadSlots = 1ull << 30;   // row slots a chunk at most: 32-bit slot indices in the kernel

// One launch counts the slots of one chunk's rows that fall into the bin window [b0, b0 + nb) of
// the flat bins id * W + q. Counts are privatised in LDS (uint32, LDS atomic adds) and flushed
// once per workgroup. Invariant: a chunk has fewer than 2^31 row slots (kLoadSlots), so no uint32
// LDS bin can overflow within one launch; the global counters are 64-bit because n is.
// Few bins: with nb << the LDS words given, 2^cl copies of the window are kept (bin b of copy c
// at word (b << cl) + c, c = lane & (2^cl - 1): with 64 copies every lane of a wave has a bank of
// its own), so that the lanes of a wave do not serialise on a handful of words; the flush sums
// the copies (rotated by the thread index, so that the threads of a wave read different banks).
// Flush: thread t adds bin t, t + 1024, ...: a wave-instruction covers 64 contiguous 8-B
// counters (512 contiguous bytes), minus the lanes whose bin is zero.
// WT: the row width when it is 1..4 (a constant divisor for the slot's q), 0: any width.
template <int WT>
__global__ __launch_bounds__(kLoadThreads) void k_owner_load(const uint32_t* __restrict__ rows, uint32_t nslots,
                                                             uint32_t Wrt, uint64_t b0, uint32_t nb, uint32_t cl,
                                                             unsigned long long* __restrict__ load) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_bins[];
    const uint32_t W = WT ? (uint32_t)WT : Wrt;
    const uint32_t tid = threadIdx.x;
    const uint32_t copy = tid & ((1u << cl) - 1u);
    const uint32_t words = nb << cl;
    for (uint32_t i = tid; i < words; i += kLoadThreads) s_bins[i] = 0;
    __syncthreads();
    auto count = [&](uint32_t id, uint32_t q) {
        if (id == NIL) return;
        const uint64_t bin = (uint64_t)id * W + q - b0;  // (below b0: wraps past nb)
        if (bin < (uint64_t)nb) atomicAdd(&s_bins[((uint32_t)bin << cl) + copy], 1u);
    };
    auto count4 = [&](const u32x4 r, uint32_t v) {
        uint32_t q = (v * 4u) % W;  // (nslots < 2^31: no wrap)
        count(r.x, q);
        q = q + 1u == W ? 0u : q + 1u;
        count(r.y, q);
        q = q + 1u == W ? 0u : q + 1u;
        count(r.z, q);
        q = q + 1u == W ? 0u : q + 1u;
        count(r.w, q);
    };
    const uint32_t nvec = nslots >> 2;
    const u32x4* r4 = reinterpret_cast<const u32x4*>(rows);
    const uint32_t step = gridDim.x * (uint32_t)kLoadThreads;
    uint32_t v = blockIdx.x * (uint32_t)kLoadThreads + tid;
    for (; v < nvec && nvec - v > 3u * step; v += 4u * step) {  // four 16-B loads in flight a thread
        const u32x4 a = r4[v], b = r4[v + step], c = r4[v + 2u * step], d = r4[v + 3u * step];
        count4(a, v);
        count4(b, v + step);
        count4(c, v + 2u * step);
        count4(d, v + 3u * step);
    }
    for (; v < nvec; v += step) count4(r4[v], v);
    if (blockIdx.x == 0 && tid < (nslots & 3u)) {  // the last 1..3 slots
        const uint32_t s = (nvec << 2) + tid;
        count(rows[s], s % W);
    }
    __syncthreads();
    for (uint32_t b = tid; b < nb; b += kLoadThreads) {
        uint32_t sum = 0;
        for (uint32_t c = 0; c < (1u << cl); c++) sum += s_bins[(b << cl) + ((c + tid) & ((1u << cl) - 1u))];
        if (sum) atomicAdd(load + b0 + b, (unsigned long long)sum);
    }
}

// share[own[i]] += the hash values whose first token >= h is token i (token 0 also takes the
// values above the last token: lookup's wrap to the smallest token)
__global__ __launch_bounds__(256) void k_owner_share(RingView rv, unsigned long long* __restrict__ share) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rv.M) return;
    const uint64_t t = rv.tok[i];
    const uint64_t d = i ? t - rv.tok[i - 1] : t + (1ull << 32) - rv.tok[rv.M - 1];
    if (d) atomicAdd(share + rv.own[i], (unsigned long long)d);
}

// Windows past 64 KB of dynamic LDS need the opt-in, on every device that launches the kernels
// (`device` is the current device: the handle's). A refusal is an error, not a smaller window.
static void load_lds_opt_in(int device) {
    static std::mutex mu;
    static std::vector<uint8_t> done;
    std::lock_guard<std::mutex> lock(mu);
    if (device >= 0 && (size_t)device < done.size() && done[device]) return;
    const int bytes = (int)(kLoadBins * sizeof(uint32_t));
    RP_HIP(hipFuncSetAttribute((const void*)k_owner_load<0>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    RP_HIP(hipFuncSetAttribute((const void*)k_owner_load<1>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    RP_HIP(hipFuncSetAttribute((const void*)k_owner_load<2>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    RP_HIP(hipFuncSetAttribute((const void*)k_owner_load<3>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    RP_HIP(hipFuncSetAttribute((const void*)k_owner_load<4>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (device >= 0) {
        if ((size_t)device >= done.size()) done.resize((size_t)device + 1, 0);
        done[device] = 1;
    }
}

// Count one chunk's rows (cnt * W slots at ls.rows) into load[0 .. bins), window by window.
static void launch_owner_load(const uint32_t* rows, uint64_t slots, uint32_t W, uint64_t bins,
                              unsigned long long* load, int device, hipStream_t st) {
    load_lds_opt_in(device);
    RP_REQUIRE(slots < (1ull << 31), "owner_load: chunk too large");
    // RP_LOAD_BINS: the window (tests reach the multi-window path with it); never past the LDS
    const uint32_t B = (uint32_t)std::min<uint64_t>(env_pos("RP_LOAD_BINS", kLoadBins), kLoadBins);
    const bool replicate = !(getenv("RP_LOAD_COPIES") && !strcmp(getenv("RP_LOAD_COPIES"), "0"));  // A/B only
    const int cus = cu_count(device);
    for (uint64_t b0 = 0; b0 < bins; b0 += B) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(B, bins - b0);
        uint32_t cl = 0;
        if (replicate)
            while (cl < 6 && ((uint64_t)nb << (cl + 1)) <= B) cl++;
        const uint32_t words = nb << cl;
        const unsigned per_cu = words <= kLoadBins2 ? 2u : 1u;
        const uint64_t nvec = slots / 4;
        const unsigned g = (unsigned)std::max<uint64_t>(
            1, std::min<uint64_t>(env_pos("RP_LOAD_GRID", (uint64_t)cus * per_cu), (nvec + kLoadThreads - 1) / kLoadThreads));
        const size_t lds = (size_t)words * sizeof(uint32_t);
#define RP_LOADK(WT)                                                                                            \
    hipLaunchKernelGGL((k_owner_load<WT>), dim3(g), dim3(kLoadThreads), lds, st, rows, (uint32_t)slots, W, b0, \
                       nb, cl, load)
        switch (W) {
            case 1: RP_LOADK(1); break;
            case 2: RP_LOADK(2); break;
            case 3: RP_LOADK(3); break;
            case 4: RP_LOADK(4); break;
            default: RP_LOADK(0); break;
        }
#undef RP_LOADK
        RP_HIP(hipGetLastError());
    }
}

// The chunk walk. look(k0, cnt, rows) queues the lookup of keys [k0, k0 + cnt) into rows on st.
template <class Look>
static void owner_load_walk(LoadScratch& ls, uint64_t n, int32_t nrep, uint32_t id_bound, uint32_t id_cap,
                            bool counts_anything, int accumulate, unsigned long long* load, int device,
                            hipStream_t st, Look&& look) {
    RP_REQUIRE(id_cap >= id_bound, "owner_load: id_cap is below the ring's id bound (rp_ring_id_bound)");
    RP_REQUIRE(id_cap == 0 || load, "owner_load: null load buffer");
    const uint32_t W = replicas(nrep, 0).W;  // (the look callback walks with its ring's server count)
    const uint64_t bins = (uint64_t)id_cap * W;
    if (!accumulate && bins) RP_HIP(hipMemsetAsync(load, 0, bins * sizeof(uint64_t), st));
    if (n == 0 || !counts_anything || bins == 0) return;
    uint64_t chunk = std::min<uint64_t>(env_pos("RP_LOAD_CHUNK", kLoadChunk), std::max<uint64_t>(1, kLoadSlots / W));
    chunk = std::min(chunk, n);
    if (chunk > 4 && chunk < n) chunk &= ~3ull;  // later chunks of 36-byte keys start 16-B aligned when the first does
    ls.use_on(st);
    ls.rows.reserve(chunk * W);
    for (uint64_t k0 = 0; k0 < n; k0 += chunk) {
        const uint64_t cnt = std::min(chunk, n - k0);
        look(k0, cnt, ls.rows.p);
        launch_owner_load(ls.rows.p, cnt * W, W, bins, load, device, st);
    }
}

static void owner_load(Ring& r, LoadScratch& ls, const DevKeys& k, uint64_t n, int32_t nrep, uint32_t id_cap,
                       int accumulate, unsigned long long* load, hipStream_t st) {
    const Replicas rep = replicas(nrep, r.server_count);
    owner_load_walk(ls, n, nrep, r.nt.size(), id_cap, r.M != 0, accumulate, load, r.device, st,
                    [&](uint64_t k0, uint64_t cnt, uint32_t* rows) {
                        const DevKeys c = k.from(k0);
                        launch_lookupn(r, c.keys, c.off, c.stride, c.hashes, cnt, rep.np, rep.W, rows, nullptr, st);
                    });
}

// share[0 .. id_cap) on the host, through the handle's scratch
static void owner_share(const RingView& rv, LoadScratch& ls, uint32_t id_bound, uint32_t id_cap, uint64_t* share,
                        hipStream_t st) {
    RP_REQUIRE(id_cap >= id_bound, "owner_share: id_cap is below the ring's id bound (rp_ring_id_bound)");
    RP_REQUIRE(id_cap == 0 || share, "owner_share: null share buffer");
    if (id_cap == 0) return;
    ls.use_on(st);
    ls.out.reserve(id_cap);
    RP_HIP(hipMemsetAsync(ls.out.p, 0, (uint64_t)id_cap * sizeof(uint64_t), st));
    if (rv.M) {
        hipLaunchKernelGGL(k_owner_share, dim3(grid_for(rv.M, 256, 1u << 24)), dim3(256), 0, st, rv, ls.out.p);
        RP_HIP(hipGetLastError());
    }
    RP_HIP(hipMemcpyAsync(share, ls.out.p, (uint64_t)id_cap * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    RP_HIP(hipStreamSynchronize(st));
}

// ------------------------------------------------------------- moved ranges
// Which hash intervals changed hands between two ring states, without any key. lookupN depends on
// the hash only through "the first token >= h", so on every interval (u[k-1], u[k]] of the sorted
// union u of both rings' tokens (2^32-1 appended) both rows are constant: at most Mb + Ma + 1
// intervals can differ. Four launches, none of which waits on another workgroup:
//   k_ranges_merge  one thread per token of either ring (and one for the appended 2^32-1): its
//                   first-token positions (i, j) in both rings by bucket search, and its slot in
//                   the stable merge (before's tokens first among equals), where (u, i, j) go.
//                   (i, j) are lower bounds by value, so equal tokens carry equal positions.
//   k_ranges_flag   one thread per merged element k. An element whose value equals its
//                   predecessor's closes an empty interval and is skipped. Otherwise both rows are
//                   walked from (i, j) of k and of k - 1 (k - 1 carries the previous distinct
//                   value, whose interval ends where k's begins) and compared in registers:
//                   head = moved and not a continuation of k - 1's pair; tail-of-previous = k - 1
//                   moved and k does not continue it. The last element flags the final tail. Heads
//                   are counted per tile; the moved hash values are summed in full.
//   k_ranges_scan   exclusive scan of the tile totals (one workgroup, in passes with a carry).
//   k_ranges_write  heads write lo and both rows at their rank; tails write hi at (heads before
//                   them) - 1; the last element writes the count.
// Tests shrink the tile (RP_RANGES_TILE, elements a workgroup) and the scan pass (RP_RANGES_SCAN)
// so that several tiles and several scan passes run on a few thousand tokens.
constexpr int kRngThreads = 256;
constexpr int kRngScanThreads = 1024;
constexpr uint32_t kRngHead = 1u, kRngTailPrev = 2u, kRngFinal = 4u;

__global__ __launch_bounds__(kRngThreads) void k_ranges_merge(RingView bv, RingView av, uint32_t* __restrict__ val,
                                                              uint32_t* __restrict__ mi, uint32_t* __restrict__ mj) {
    const uint32_t N = bv.M + av.M;
    const uint32_t g = blockIdx.x * (uint32_t)kRngThreads + threadIdx.x;
    if (g > N) return;
    const uint32_t t = g < bv.M ? bv.tok[g] : (g < N ? av.tok[g - bv.M] : NIL);
    const uint32_t i = moved_find(bv, t), j = moved_find(av, t);
    uint32_t pos = N;
    if (g < bv.M) pos = g + j;  // + after's tokens below t
    else if (g < N) pos = (g - bv.M) + (t == NIL ? bv.M : moved_find(bv, t + 1u));  // + before's tokens <= t
    if (pos > N) return;  // (sorted arrays never get here; an unsorted one must not write out of bounds)
    val[pos] = t;
    mi[pos] = i;
    mj[pos] = j;
}

// both rows from the first-token positions (i, j); true when they differ
template <int MAXN>
__device__ __forceinline__ bool ranges_rows(const RingView& bv, int npb, const RingView& av, int npa, uint32_t i,
                                            uint32_t j, uint32_t (&rb)[MAXN], uint32_t (&ra)[MAXN]) {
    moved_walk<MAXN>(bv, i < bv.M ? i : bv.M, npb, rb);
    moved_walk<MAXN>(av, j < av.M ? j : av.M, npa, ra);
    bool d = false;
#pragma unroll
    for (int q = 0; q < MAXN; q++) d |= rb[q] != ra[q];
    return d;
}

template <int MAXN>
__global__ __launch_bounds__(kRngThreads) void k_ranges_flag(RingView bv, int npb, RingView av, int npa,
                                                             const uint32_t* __restrict__ val,
                                                             const uint32_t* __restrict__ mi,
                                                             const uint32_t* __restrict__ mj, uint32_t tile_n,
                                                             uint8_t* __restrict__ flg, uint32_t* __restrict__ tot,
                                                             unsigned long long* __restrict__ moved_hashes) {
    __shared__ uint32_t s_heads;
    __shared__ unsigned long long s_moved;
    const uint32_t N = bv.M + av.M, tid = threadIdx.x;
    const uint32_t k = blockIdx.x * tile_n + tid;
    if (tid == 0) {
        s_heads = 0;
        s_moved = 0;
    }
    __syncthreads();
    uint32_t f = 0;
    if (tid < tile_n && k <= N) {
        const uint32_t u = val[k], up = k ? val[k - 1] : 0u;
        const bool rep = k == 0 || u != up, fin = k == N;
        if (rep || fin) {
            uint32_t rb[MAXN], ra[MAXN];
            const bool moved = ranges_rows<MAXN>(bv, npb, av, npa, mi[k], mj[k], rb, ra);
            bool prev_moved = false, cont = false;
            if (rep && k > 0) {
                uint32_t pb[MAXN], pa[MAXN];
                prev_moved = ranges_rows<MAXN>(bv, npb, av, npa, mi[k - 1], mj[k - 1], pb, pa);
                bool same = true;
#pragma unroll
                for (int q = 0; q < MAXN; q++) same &= (pb[q] == rb[q]) & (pa[q] == ra[q]);
                cont = prev_moved & moved & same;
            }
            if (rep && moved && !cont) f |= kRngHead;
            if (rep && prev_moved && !cont) f |= kRngTailPrev;
            if (fin && moved) f |= kRngFinal;
            if (rep && moved) atomicAdd(&s_moved, k ? (unsigned long long)(u - up) : (unsigned long long)u + 1ull);
        }
        flg[k] = (uint8_t)f;
    }
    const uint64_t m = __ballot(f & kRngHead);
    if ((tid & 63u) == 0 && m) atomicAdd(&s_heads, (uint32_t)__popcll(m));
    __syncthreads();
    if (tid == 0) {
        tot[blockIdx.x] = s_heads;
        if (s_moved) atomicAdd(moved_hashes, s_moved);
    }
}

__global__ __launch_bounds__(kRngScanThreads) void k_ranges_scan(uint32_t* __restrict__ tot, uint32_t ntiles,
                                                                 uint32_t pass) {
    __shared__ uint32_t s_w[kRngScanThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < ntiles; base += pass) {
        const bool in = tid < pass && tid < ntiles - base;
        const uint32_t x = in ? tot[base + tid] : 0u;
        uint32_t inc = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d);
            if (lane >= (uint32_t)d) inc += y;
        }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint32_t wpre = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kRngScanThreads / 64; w++) {
            const uint32_t c = s_w[w];
            wpre += (uint32_t)w < wave ? c : 0u;
            total += c;
        }
        if (in) tot[base + tid] = carry + wpre + inc - x;
        carry += total;
        __syncthreads();
    }
}

template <int MAXN>
__global__ __launch_bounds__(kRngThreads) void k_ranges_write(RingView bv, int npb, RingView av, int npa,
                                                              const uint32_t* __restrict__ val,
                                                              const uint32_t* __restrict__ mi,
                                                              const uint32_t* __restrict__ mj,
                                                              const uint8_t* __restrict__ flg,
                                                              const uint32_t* __restrict__ off, uint32_t tile_n,
                                                              uint32_t W, uint32_t cap, uint32_t* __restrict__ lo,
                                                              uint32_t* __restrict__ hi, uint32_t* __restrict__ brow,
                                                              uint32_t* __restrict__ arow, uint32_t* __restrict__ count) {
    __shared__ uint32_t s_w[kRngThreads / 64];
    const uint32_t N = bv.M + av.M, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t k = blockIdx.x * tile_n + tid;
    const bool active = tid < tile_n && k <= N;
    const uint32_t f = active ? flg[k] : 0u;
    const bool head = f & kRngHead;
    const uint64_t m = __ballot(head);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t excl = off[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < kRngThreads / 64; w++) excl += (uint32_t)w < wave ? s_w[w] : 0u;
    // excl = heads before this element; every write is bounded by cap
    if ((f & kRngTailPrev) && excl > 0 && excl - 1u < cap) hi[excl - 1u] = val[k - 1];
    if (head && excl < cap) {
        lo[excl] = k ? val[k - 1] + 1u : 0u;
        if (brow || arow) {
            uint32_t rb[MAXN], ra[MAXN];
            ranges_rows<MAXN>(bv, npb, av, npa, mi[k], mj[k], rb, ra);
#pragma unroll
            for (int q = 0; q < MAXN; q++) {
                if ((uint32_t)q < W) {
                    if (brow) brow[(uint64_t)excl * W + q] = rb[q];
                    if (arow) arow[(uint64_t)excl * W + q] = ra[q];
                }
            }
        }
    }
    if (active && k == N) {
        const uint32_t total = excl + (head ? 1u : 0u);
        if ((f & kRngFinal) && total > 0 && total - 1u < cap) hi[total - 1u] = NIL;  // the run that ends at 2^32-1
        *count = total;
    }
}

// Ranges between the states (bv, sc_b servers) and (av, sc_a servers); outputs as
// rp_ring_moved_ranges_dev documents. Everything is queued on st.
static void moved_ranges(const RingView& bv, uint32_t sc_b, const RingView& av, uint32_t sc_a, RangeScratch& ws,
                         int32_t nrep, uint32_t cap, uint32_t* lo, uint32_t* hi, uint32_t* brow, uint32_t* arow,
                         uint32_t* count, uint64_t* moved_hashes, hipStream_t st) {
    RP_REQUIRE(nrep <= 8, "moved_ranges: nrep is at most 8 (the rows are compared in registers)");
    RP_REQUIRE(count && moved_hashes, "moved_ranges: null count");
    RP_REQUIRE(cap == 0 || (lo && hi), "moved_ranges: null range buffer");
    RP_REQUIRE((uint64_t)bv.M + av.M < (1ull << 31), "moved_ranges: more than 2^31 tokens");
    RP_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), st));
    RP_HIP(hipMemsetAsync(moved_hashes, 0, sizeof(uint64_t), st));
    if (bv.M == 0 && av.M == 0) return;
    const uint32_t n = bv.M + av.M + 1u;  // merged elements
    const uint32_t tile_n = (uint32_t)std::min<uint64_t>(env_pos("RP_RANGES_TILE", kRngThreads), kRngThreads);
    const uint32_t pass = (uint32_t)std::min<uint64_t>(env_pos("RP_RANGES_SCAN", kRngScanThreads), kRngScanThreads);
    const uint32_t ntiles = (n + tile_n - 1u) / tile_n;
    ws.use_on(st);
    ws.val.reserve(n);
    ws.mi.reserve(n);
    ws.mj.reserve(n);
    ws.flg.reserve(n);
    ws.tot.reserve(ntiles);
    const int npb = replicas(nrep, sc_b).np;
    const auto [npa, W] = replicas(nrep, sc_a);
    hipLaunchKernelGGL(k_ranges_merge, dim3((n + kRngThreads - 1) / kRngThreads), dim3(kRngThreads), 0, st, bv, av,
                       ws.val.p, ws.mi.p, ws.mj.p);
    RP_HIP(hipGetLastError());
    unsigned long long* mh = reinterpret_cast<unsigned long long*>(moved_hashes);
#define RP_RANGES(MAXN)                                                                                              \
    do {                                                                                                             \
        hipLaunchKernelGGL((k_ranges_flag<MAXN>), dim3(ntiles), dim3(kRngThreads), 0, st, bv, npb, av, npa,          \
                           ws.val.p, ws.mi.p, ws.mj.p, tile_n, ws.flg.p, ws.tot.p, mh);                              \
        RP_HIP(hipGetLastError());                                                                                   \
        hipLaunchKernelGGL(k_ranges_scan, dim3(1), dim3(kRngScanThreads), 0, st, ws.tot.p, ntiles, pass);            \
        RP_HIP(hipGetLastError());                                                                                   \
        hipLaunchKernelGGL((k_ranges_write<MAXN>), dim3(ntiles), dim3(kRngThreads), 0, st, bv, npb, av, npa,         \
                           ws.val.p, ws.mi.p, ws.mj.p, ws.flg.p, ws.tot.p, tile_n, W, cap, lo, hi, brow, arow,       \
                           count);                                                                                   \
        RP_HIP(hipGetLastError());                                                                                   \
    } while (0)
    if (W == 1) RP_RANGES(1);
    else if (W <= 4) RP_RANGES(4);
    else RP_RANGES(8);
#undef RP_RANGES
}

// The host form: the same through the handle's scratch, then two copies (the counts, then the
// entries that exist).
static void host_moved_ranges(const RingView& bv, uint32_t sc_b, const RingView& av, uint32_t sc_a, RangeScratch& ws,
                              int32_t nrep, uint32_t cap, uint32_t* lo, uint32_t* hi, uint32_t* brows, uint32_t* arows,
                              uint32_t* count, uint64_t* moved_hashes, hipStream_t st) {
    RP_REQUIRE(nrep <= 8, "moved_ranges: nrep is at most 8 (the rows are compared in registers)");
    RP_REQUIRE(count && moved_hashes, "moved_ranges: null count");
    RP_REQUIRE(cap == 0 || (lo && hi), "moved_ranges: null range buffer");
    RP_REQUIRE((uint64_t)bv.M + av.M < (1ull << 31), "moved_ranges: more than 2^31 tokens");
    // io = [moved_hashes 2 | count 1 | pad 1 | lo c | hi c | before rows c*W | after rows c*W]
    const uint64_t c = std::min<uint64_t>(cap, (uint64_t)bv.M + av.M + 1u), W = replicas(nrep, sc_a).W;
    ws.use_on(st);
    ws.io.reserve(4 + c * (2 + 2 * W));
    uint32_t* dlo = ws.io.p + 4;
    uint32_t* dhi = dlo + c;
    uint32_t* dbr = dhi + c;
    uint32_t* dar = dbr + c * W;
    moved_ranges(bv, sc_b, av, sc_a, ws, nrep, (uint32_t)c, c ? dlo : nullptr, c ? dhi : nullptr,
                 brows ? dbr : nullptr, arows ? dar : nullptr, ws.io.p + 2, reinterpret_cast<uint64_t*>(ws.io.p), st);
    uint32_t head[4] = {0, 0, 0, 0};
    RP_HIP(hipMemcpyAsync(head, ws.io.p, sizeof(head), hipMemcpyDeviceToHost, st));
    RP_HIP(hipStreamSynchronize(st));
    *count = head[2];
    *moved_hashes = (uint64_t)head[0] | ((uint64_t)head[1] << 32);
    const uint64_t m = std::min<uint64_t>(head[2], c);
    if (m) {
        RP_HIP(hipMemcpyAsync(lo, dlo, m * 4, hipMemcpyDeviceToHost, st));
        RP_HIP(hipMemcpyAsync(hi, dhi, m * 4, hipMemcpyDeviceToHost, st));
        if (brows) RP_HIP(hipMemcpyAsync(brows, dbr, m * W * 4, hipMemcpyDeviceToHost, st));
        if (arows) RP_HIP(hipMemcpyAsync(arows, dar, m * W * 4, hipMemcpyDeviceToHost, st));
        RP_HIP(hipStreamSynchronize(st));
    }
}

// ------------------------------------------------------------- routing agreement
// Key owners under many views of one base ring at once (rp_ring_route_views*). A view allows a
// subset of the ring's servers; owner(v, h) is the owner of the first token at or after h's
// position, walking cyclically, whose server view v allows. Two launches:
//   k_route_pack  transposes the caller's byte rows rows[v][col[id]] & bit into bit planes
//                 plane[id][PW] (bit b of word w: view 64 w + b allows server id; tail bits and
//                 servers without tokens are zero). One thread per (id, word): it reads the 64
//                 rows' bytes at its column, so a workgroup's 256 consecutive ids read 256
//                 contiguous bytes of a row per step when col is the identity. It also writes the
//                 truth byte per id, the active words, any[w] = OR of the planes over the ids
//                 (views that allow nobody are answered RP_NULL_ID without a walk) and whether the
//                 truth allows anybody.
//   k_route       a wave takes 64 keys: each lane hashes one, finds its position (moved_find) and
//                 walks to its owner under the truth. Then the wave walks the keys one by one with
//                 one lane per view word: the step's owner is wave-uniform, a lane whose word has
//                 views left loads plane[owner][word], and the views it answers are classed as
//                 agreeing, wrong or lost against the truth and leave the word. A repeated owner
//                 answers nothing new. The first step's owner is read with the position (one
//                 load a lane, not one a key); after the first step the walk issues four steps'
//                 plane loads together (the positions are known in advance). Counts go to uint32 LDS
//                 counters per view (one LDS atomic per wrong view: disagreements are rare) and
//                 are flushed with 64-bit global atomics; a launch takes fewer than 2^32 keys.
//                 blockIdx.y is the block of up to 64 view words the workgroup's LDS counts.
constexpr int kRouteThreads = 512;
constexpr int kRoutePackThreads = 256;
constexpr uint32_t kRouteVBlock = 4096;       // views a block (RP_ROUTE_VBLOCK): 64 words, one a lane
constexpr uint64_t kRouteChunk = 1ull << 31;  // keys a launch: the uint32 LDS counters cannot overflow

__global__ __launch_bounds__(kRoutePackThreads) void k_route_pack(
    const uint8_t* __restrict__ rows, uint64_t row_stride, uint8_t bit, uint32_t V, const uint32_t* __restrict__ col,
    uint32_t idb, const uint8_t* __restrict__ inring, uint32_t inring_n, const uint8_t* __restrict__ truth,
    const uint8_t* __restrict__ active, uint32_t PW, unsigned long long* __restrict__ plane,
    unsigned long long* __restrict__ any, unsigned long long* __restrict__ act, unsigned long long* __restrict__ tany,
    uint8_t* __restrict__ tr) {
    const uint32_t id = blockIdx.x * (uint32_t)kRoutePackThreads + threadIdx.x, w = blockIdx.y, lane = threadIdx.x & 63;
    const bool inr = id < idb && id < inring_n && inring[id] != 0;
    uint32_t c = NIL;
    if (inr) {
        c = col ? col[id] : id;
        if ((uint64_t)c >= row_stride) c = NIL;  // (never read past a row)
    }
    const uint32_t vb = w * 64u;
    const uint32_t nv = V > vb ? (V - vb < 64u ? V - vb : 64u) : 0u;
    unsigned long long word = 0;
    if (c != NIL) {
        const uint8_t* p = rows + (uint64_t)vb * row_stride + c;
#pragma unroll 8
        for (uint32_t b = 0; b < nv; b++)
            word |= (unsigned long long)((p[(uint64_t)b * row_stride] & bit) != 0) << b;
    }
    if (id < idb) plane[(uint64_t)id * PW + w] = word;
    unsigned long long r = word;
#pragma unroll
    for (int o = 32; o; o >>= 1) r |= __shfl_xor(r, o);
    if (lane == 0 && r) atomicOr(any + w, r);
    if (w == 0) {
        const bool t = truth ? (c != NIL && (truth[c] & bit) != 0) : inr;
        if (id < idb) tr[id] = t ? 1 : 0;
        const unsigned long long m = __ballot(t);
        if (lane == 0 && m) atomicOr(tany, 1ull);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const uint32_t v = vb + lane;
        const unsigned long long m = __ballot(v < V && (active ? active[v] != 0 : true));
        if (lane == 0) act[w] = m;
    }
}

// FIXED: 36-byte keys at stride 36 from a 4-byte aligned base (nine dword loads a lane).
// OWN: the per-view owners are written (the diagnostic output), and inactive views are walked too.
template <bool FIXED, bool OWN>
__global__ __launch_bounds__(kRouteThreads) void k_route(
    const uint8_t* __restrict__ keys, const uint64_t* __restrict__ off, uint32_t stride,
    const uint32_t* __restrict__ hashes, uint32_t n, RingView rv, const unsigned long long* __restrict__ plane,
    const unsigned long long* __restrict__ any, const unsigned long long* __restrict__ act,
    const unsigned long long* __restrict__ tany, const uint8_t* __restrict__ tr, uint32_t PW, uint32_t V,
    uint32_t VBW, unsigned long long* __restrict__ wrong, unsigned long long* __restrict__ lost,
    uint32_t* __restrict__ key_wrong, uint32_t* __restrict__ truth_owner, uint32_t* __restrict__ owners) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_route[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t w0 = blockIdx.y * VBW;
    const uint32_t nw = PW - w0 < VBW ? PW - w0 : VBW;  // this block's view words (<= 64)
    uint32_t* s_wrong = s_route;
    uint32_t* s_lost = s_route + nw * 64u;
    for (uint32_t i = tid; i < nw * 128u; i += kRouteThreads) s_route[i] = 0;
    __syncthreads();
    const bool on = lane < nw;
    const uint32_t w = w0 + (on ? lane : 0u);
    unsigned long long valid = 0;
    if (on && V > w * 64u) valid = V - w * 64u >= 64u ? ~0ull : ((1ull << (V - w * 64u)) - 1ull);
    const unsigned long long actw = on ? act[w] : 0ull;
    const unsigned long long anyw = on ? any[w] : 0ull;
    const unsigned long long walked = OWN ? valid : (valid & actw);
    const bool has_truth = *tany != 0;
    const uint32_t M = rv.M;
    const uint32_t step = gridDim.x * (uint32_t)kRouteThreads;
    for (uint64_t base = ((uint64_t)blockIdx.x * (kRouteThreads / 64) + wave) * 64u; base < n; base += step) {
        const uint32_t cnt = n - base < 64u ? (uint32_t)(n - base) : 64u;
        uint32_t pos = 0, tk = NIL, o0 = 0;
        if (lane < cnt) {
            const uint64_t k = base + lane;
            const uint32_t h = FIXED ? key_hash36(reinterpret_cast<const uint32_t*>(keys + k * 36u))
                                     : key_hash(keys, off, stride, hashes, k);
            pos = moved_find(rv, h);
            if (pos >= M) pos = 0;
            o0 = rv.own[pos];
            if (has_truth) {  // (some owner in the ring is allowed: at most M steps)
                uint32_t j = pos;
                for (uint32_t s = 0; s < M; s++) {
                    const uint32_t o = rv.own[j];
                    if (tr[o]) {
                        tk = o;
                        break;
                    }
                    j = j + 1u == M ? 0u : j + 1u;
                }
            }
            if (blockIdx.y == 0 && truth_owner) truth_owner[k] = tk;
        }
        for (uint32_t kk = 0; kk < cnt; kk++) {
            const uint32_t i = __shfl(pos, (int)kk), t = __shfl(tk, (int)kk), first = __shfl(o0, (int)kk);
            unsigned long long rem = walked & anyw, wr = 0, lo = 0;
            if (t != NIL) wr = walked & ~anyw;  // views that allow nobody answer null
            uint32_t* orow = OWN ? owners + (base + kk) * (uint64_t)V + (uint64_t)w * 64u : nullptr;
            auto apply = [&](uint32_t o, unsigned long long p) {
                unsigned long long hit = rem & p;
                if (hit) {
                    rem &= ~hit;
                    if (o != t) {
                        wr |= hit;
                        if (!tr[o]) lo |= hit;
                    }
                    if constexpr (OWN) {
                        while (hit) {
                            orow[__builtin_ctzll(hit)] = o;
                            hit &= hit - 1ull;
                        }
                    }
                }
            };
            if (rem) apply(first, plane[(uint64_t)first * PW + w]);
            uint32_t j = i + 1u == M ? 0u : i + 1u;
            for (uint32_t steps = 1; steps < M && __ballot(rem != 0); steps += 4u) {
                uint32_t o4[4];
                unsigned long long p4[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    o4[q] = rv.own[j];
                    j = j + 1u == M ? 0u : j + 1u;
                }
                if (rem) {
#pragma unroll
                    for (int q = 0; q < 4; q++) p4[q] = plane[(uint64_t)o4[q] * PW + w];
#pragma unroll
                    for (int q = 0; q < 4; q++) apply(o4[q], p4[q]);  // (steps past M revisit answered owners)
                }
            }
            if (t != NIL) wr |= rem;  // (no allowed owner after M steps: null)
            wr &= actw;
            lo &= actw;
            if (wr) {
                if (key_wrong) atomicAdd(key_wrong + base + kk, (uint32_t)__popcll(wr));
                while (wr) {
                    atomicAdd(&s_wrong[lane * 64u + (uint32_t)__builtin_ctzll(wr)], 1u);
                    wr &= wr - 1ull;
                }
                while (lo) {
                    atomicAdd(&s_lost[lane * 64u + (uint32_t)__builtin_ctzll(lo)], 1u);
                    lo &= lo - 1ull;
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < nw * 64u; i += kRouteThreads) {
        const uint64_t v = (uint64_t)w0 * 64u + i;
        if (v >= V) break;
        const uint32_t a = s_wrong[i], b = s_lost[i];
        if (a && wrong) atomicAdd(wrong + v, (unsigned long long)a);
        if (b && lost) atomicAdd(lost + v, (unsigned long long)b);
    }
}

// Outputs as rp_ring_route_views_dev documents; everything is queued on st.
static void route_views(Ring& r, const DevKeys& k, uint64_t n, const uint8_t* rows, uint64_t row_stride, uint8_t bit,
                        uint32_t V, const uint32_t* col, uint32_t id_cap, const uint8_t* truth, const uint8_t* active,
                        int accumulate, uint64_t* wrong, uint64_t* lost, uint32_t* key_wrong, uint32_t* truth_owner,
                        uint32_t* owners, hipStream_t st) {
    const uint32_t idb = r.nt.size();
    RP_REQUIRE(id_cap >= idb, "route_views: id_cap is below the ring's id bound (rp_ring_id_bound)");
    RP_REQUIRE(n == 0 || ((k.keys != nullptr) != (k.hashes != nullptr)),
               "route_views: exactly one of the key buffer and the hash buffer");
    RP_REQUIRE(n == 0 || k.hashes || k.stride || k.off, "route_views: null key offsets");
    RP_REQUIRE(V == 0 || rows, "route_views: null view rows");
    RP_REQUIRE(bit != 0, "route_views: bit is zero");
    RP_REQUIRE(V == 0 || col || row_stride >= id_cap, "route_views: without a column map row_stride covers id_cap");
    const uint32_t PW = V ? (V + 63u) / 64u : 1u;
    RP_REQUIRE(PW <= 65535u, "route_views: at most 4,194,240 views a call");
    // the ring is rebuilt on r.st; make the caller's stream wait for it
    if (st != r.st) RP_HIP(hipStreamSynchronize(r.st));
    if (!accumulate && V) {
        if (wrong) RP_HIP(hipMemsetAsync(wrong, 0, (uint64_t)V * 8, st));
        if (lost) RP_HIP(hipMemsetAsync(lost, 0, (uint64_t)V * 8, st));
    }
    if (n == 0) return;
    if (key_wrong) RP_HIP(hipMemsetAsync(key_wrong, 0, n * 4, st));
    if (owners && V) RP_HIP(hipMemsetAsync(owners, 0xFF, n * V * 4, st));  // RP_NULL_ID until a view answers
    if (r.M == 0) {  // every owner is null, the truth's too
        if (truth_owner) RP_HIP(hipMemsetAsync(truth_owner, 0xFF, n * 4, st));
        return;
    }
    RouteScratch& ws = r.route_ws;
    ws.use_on(st);
    ws.plane.reserve((uint64_t)idb * PW);
    ws.meta.reserve(2ull * PW + 1);
    ws.tr.reserve(idb);
    unsigned long long* any = ws.meta.p;
    unsigned long long* act = any + PW;
    unsigned long long* tany = act + PW;
    RP_HIP(hipMemsetAsync(ws.meta.p, 0, (2ull * PW + 1) * 8, st));
    hipLaunchKernelGGL(k_route_pack, dim3((idb + kRoutePackThreads - 1) / kRoutePackThreads, PW),
                       dim3(kRoutePackThreads), 0, st, rows, row_stride, bit, V, col, idb, r.d_inring.p, r.inring_n,
                       truth, active, PW, ws.plane.p, any, act, tany, ws.tr.p);
    RP_HIP(hipGetLastError());
    uint64_t vblock = std::min<uint64_t>(env_pos("RP_ROUTE_VBLOCK", kRouteVBlock), kRouteVBlock);
    vblock = std::max<uint64_t>(64, vblock & ~63ull);
    const uint32_t VBW = (uint32_t)(vblock / 64), nvb = (PW + VBW - 1) / VBW;
    const size_t lds = (size_t)std::min(VBW, PW) * 128u * sizeof(uint32_t);
    const bool fixed36 = k.fixed36();
    const RingView rv = r.view();
    const uint64_t gcap = (uint64_t)cu_count(r.device) * 4;  // 512 threads at <= 64 VGPRs: four workgroups a CU
    for (uint64_t k0 = 0; k0 < n; k0 += kRouteChunk) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(kRouteChunk, n - k0);
        const unsigned g = (unsigned)std::max<uint64_t>(
            1, std::min<uint64_t>(gcap, ((uint64_t)cnt + kRouteThreads - 1) / kRouteThreads));
        const DevKeys c = k.from(k0);
#define RP_ROUTE(FIXED, OWN)                                                                                       \
    hipLaunchKernelGGL((k_route<FIXED, OWN>), dim3(g, nvb), dim3(kRouteThreads), lds, st, c.keys, c.off, c.stride, \
                       c.hashes, cnt, rv, ws.plane.p, any, act, tany, ws.tr.p, PW, V, VBW,                         \
                       reinterpret_cast<unsigned long long*>(wrong), reinterpret_cast<unsigned long long*>(lost),  \
                       key_wrong ? key_wrong + k0 : nullptr, truth_owner ? truth_owner + k0 : nullptr,             \
                       owners ? owners + k0 * V : nullptr)
        if (fixed36) {
            if (owners) RP_ROUTE(true, true);
            else RP_ROUTE(true, false);
        } else {
            if (owners) RP_ROUTE(false, true);
            else RP_ROUTE(false, false);
        }
#undef RP_ROUTE
        RP_HIP(hipGetLastError());
    }
}

// ------------------------------------------------------------- routing agreement over the hash space
// On how many of the 2^32 hash values every view disagrees with the truth (rp_ring_route_share*),
// without any key. owner(v, h) and t(h) are constant on the interval of each token position, so
// the answer is a sum of interval lengths, and the wrong / lost bits of position k follow from
// those of position k + 1 (cyclically), bitwise in a 64-view plane word:
//   W_k = (P_k ^ T_k)  | (~P_k & ~T_k & W_{k+1})      P_k: the view allows own[k] (k_route_pack's
//   L_k = (P_k & ~T_k) | (~P_k        & L_{k+1})      planes), T_k: the truth does (its tr byte)
// Both are generate / propagate recurrences x_k = g_k | (p_k & x_{k+1}); pairs compose by
// (g, p) o (g', p') = (g | p & g', p & p'). The ring is cut into chunks of C positions. After
// k_route_pack, three launches, none of which waits on another workgroup:
//   k_share_reduce  one thread per (chunk, view word) composes its chunk's (g, p) for W and for L,
//                   walking the chunk upwards; a wave's lanes are consecutive words of one chunk, so
//                   its plane reads are contiguous. Eight positions' loads are issued together.
//   k_share_carry   one thread per view word composes the chunk aggregates from the last chunk to
//                   the first. The value entering position M - 1 from position 0 is G, the generate
//                   word of the whole ring: a bit that propagates all the way round has no generate
//                   anywhere (the view allows nobody, and for W neither does the truth) and is 0.
//                   Then it writes every chunk's carry-in: the two words entering its last position.
//   k_share_apply   one wave per (chunk, view word), one lane per view. The wave takes 64 positions
//                   at a time from the chunk's end: lane j loads position top - 1 - j's owner, truth
//                   byte, plane word and interval length (one coalesced and one gathered load each),
//                   and the 64 steps read them lane by lane (v_readlane: wave-uniform). Each lane
//                   keeps its own W and L bit and adds the length to two uint64 registers; at the end
//                   of the chunk one 64-bit atomic per non-zero (view, counter). POS: a ballot of
//                   the active W bits per step, its popcount kept by the step's lane and added to
//                   pos_wrong with one atomic per position and view word.
// The cost is M * PW wave steps whatever the views or the truth look like.
constexpr int kShareThreads = 256;          // k_share_reduce and k_share_apply: four waves
constexpr int kShareCarryThreads = 64;      // k_share_carry
constexpr uint32_t kShareMinChunk = 64;     // positions: one batch of k_share_apply
constexpr uint64_t kShareMaxWords = 1ull << 24;  // chunks * view words the aggregates may take (768 MB)

__global__ __launch_bounds__(kShareThreads) void k_share_reduce(
    const uint32_t* __restrict__ own, uint32_t M, uint32_t C, const unsigned long long* __restrict__ plane,
    const uint8_t* __restrict__ tr, uint32_t PW, unsigned long long* __restrict__ agg) {
    const uint32_t w = (blockIdx.y * (uint32_t)(kShareThreads / 64) + (threadIdx.x >> 6)) * 64u + (threadIdx.x & 63);
    if (w >= PW) return;
    const uint32_t c = blockIdx.x;
    const uint64_t lo = (uint64_t)c * C, hi = lo + C < M ? lo + C : M;
    unsigned long long gw = 0, pw = ~0ull, gl = 0, pl = ~0ull;
    for (uint64_t k = lo; k < hi; k += 8) {
        uint32_t o[8];
        unsigned long long p[8];
        uint8_t t[8];
#pragma unroll
        for (int q = 0; q < 8; q++) o[q] = own[k + q < hi ? k + q : hi - 1];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            p[q] = plane[(uint64_t)o[q] * PW + w];
            t[q] = tr[o[q]];
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
            if (k + q >= hi) break;
            const unsigned long long T = t[q] ? ~0ull : 0ull, P = p[q];
            gw |= pw & (P ^ T);
            pw &= ~P & ~T;
            gl |= pl & (P & ~T);
            pl &= ~P;
        }
    }
    unsigned long long* a = agg + (uint64_t)c * 4u * PW + w;
    a[0] = gw;
    a[PW] = pw;
    a[2ull * PW] = gl;
    a[3ull * PW] = pl;
}

__global__ __launch_bounds__(kShareCarryThreads) void k_share_carry(
    const unsigned long long* __restrict__ agg, uint32_t nchunks, uint32_t PW, unsigned long long* __restrict__ carry) {
    const uint32_t w = blockIdx.x * (uint32_t)kShareCarryThreads + threadIdx.x;
    if (w >= PW) return;
    unsigned long long xw = 0, xl = 0;  // the whole ring's generate words
#pragma unroll 4
    for (uint32_t c = nchunks; c-- > 0;) {
        const unsigned long long* a = agg + (uint64_t)c * 4u * PW + w;
        xw = a[0] | (a[PW] & xw);
        xl = a[2ull * PW] | (a[3ull * PW] & xl);
    }
#pragma unroll 4
    for (uint32_t c = nchunks; c-- > 0;) {
        const unsigned long long* a = agg + (uint64_t)c * 4u * PW + w;
        carry[(uint64_t)c * 2u * PW + w] = xw;
        carry[((uint64_t)c * 2u + 1u) * PW + w] = xl;
        xw = a[0] | (a[PW] & xw);
        xl = a[2ull * PW] | (a[3ull * PW] & xl);
    }
}

__device__ __forceinline__ unsigned long long share_lane64(unsigned long long v, uint32_t j) {
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j);
    return ((unsigned long long)b << 32) | a;
}

template <bool POS>
__global__ __launch_bounds__(kShareThreads) void k_share_apply(
    RingView rv, uint32_t C, const unsigned long long* __restrict__ plane, const unsigned long long* __restrict__ act,
    const uint8_t* __restrict__ tr, const unsigned long long* __restrict__ carry, uint32_t PW,
    unsigned long long* __restrict__ wrong, unsigned long long* __restrict__ lost, uint32_t* __restrict__ pos_wrong) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.y * (uint32_t)(kShareThreads / 64) + (threadIdx.x >> 6);
    if (w >= PW) return;
    const uint32_t c = blockIdx.x, M = rv.M;
    const uint64_t lo = (uint64_t)c * C, hi = lo + C < M ? lo + C : M;
    const bool on = (act[w] >> lane) & 1ull;
    bool W = (carry[(uint64_t)c * 2u * PW + w] >> lane) & 1ull;
    bool L = (carry[((uint64_t)c * 2u + 1u) * PW + w] >> lane) & 1ull;
    unsigned long long aw = 0, al = 0;
    for (uint64_t top = hi; top > lo;) {
        const uint32_t cnt = top - lo < 64u ? (uint32_t)(top - lo) : 64u;
        const uint32_t k = (uint32_t)(top - 1u) - (lane < cnt ? lane : 0u);
        const uint32_t o = rv.own[k];
        const uint32_t t = tr[o];
        const unsigned long long p = plane[(uint64_t)o * PW + w];
        const uint64_t tk = rv.tok[k];
        const unsigned long long len = k ? tk - rv.tok[k - 1] : tk + (1ull << 32) - rv.tok[M - 1];
        uint32_t pc = 0;
        for (uint32_t j = 0; j < cnt; j++) {
            const bool P = (share_lane64(p, j) >> lane) & 1ull;
            if (__builtin_amdgcn_readlane((int)t, (int)j)) {
                W = !P;
                L = !P && L;
            } else {
                W = P || W;
                L = P || L;
            }
            const unsigned long long lj = share_lane64(len, j);
            if (on && W) aw += lj;
            if (on && L) al += lj;
            if constexpr (POS) {
                const unsigned long long m = __ballot(on && W);
                if (lane == j) pc = (uint32_t)__popcll(m);
            }
        }
        if constexpr (POS) {
            if (lane < cnt && pc) atomicAdd(pos_wrong + k, pc);
        }
        top -= cnt;
    }
    const uint64_t v = (uint64_t)w * 64u + lane;  // (below n_views wherever `on`)
    if (aw && wrong) atomicAdd(wrong + v, aw);
    if (al && lost) atomicAdd(lost + v, al);
}

// Outputs as rp_ring_route_share_dev documents; everything is queued on st.
static void route_share(Ring& r, const uint8_t* rows, uint64_t row_stride, uint8_t bit, uint32_t V, const uint32_t* col,
                        uint32_t id_cap, const uint8_t* truth, const uint8_t* active, int accumulate, uint64_t* wrong,
                        uint64_t* lost, uint32_t* pos_wrong, uint32_t pos_cap, hipStream_t st) {
    const uint32_t idb = r.nt.size(), M = r.M;
    RP_REQUIRE(id_cap >= idb, "route_share: id_cap is below the ring's id bound (rp_ring_id_bound)");
    RP_REQUIRE(V == 0 || rows, "route_share: null view rows");
    RP_REQUIRE(bit != 0, "route_share: bit is zero");
    RP_REQUIRE(V == 0 || col || row_stride >= id_cap, "route_share: without a column map row_stride covers id_cap");
    RP_REQUIRE(!pos_wrong || pos_cap >= M, "route_share: pos_cap is below the token count");
    const uint32_t PW = V ? (V + 63u) / 64u : 1u;
    RP_REQUIRE(PW <= 65535u, "route_share: at most 4,194,240 views a call");
    const uint64_t knob = env_pos("RP_SHARE_CHUNK", 0);  // positions a chunk (read once per call)
    // the ring is rebuilt on r.st; make the caller's stream wait for it
    if (st != r.st) RP_HIP(hipStreamSynchronize(r.st));
    if (!accumulate && V) {
        if (wrong) RP_HIP(hipMemsetAsync(wrong, 0, (uint64_t)V * 8, st));
        if (lost) RP_HIP(hipMemsetAsync(lost, 0, (uint64_t)V * 8, st));
    }
    if (M == 0) return;  // every owner is null, the truth's too
    if (pos_wrong) RP_HIP(hipMemsetAsync(pos_wrong, 0, (uint64_t)M * 4, st));
    if (V == 0 || (!wrong && !lost && !pos_wrong)) return;
    // chunks: four a compute unit at M = 10^6, at least one batch of k_share_apply each, and no
    // more aggregates than kShareMaxWords whatever the knob says
    const uint64_t want = 4ull * cu_count(r.device);
    uint64_t C = knob ? knob : std::max<uint64_t>(kShareMinChunk, (M + want - 1) / want);
    C = std::min<uint64_t>(std::max<uint64_t>(C, ((uint64_t)M * PW + kShareMaxWords - 1) / kShareMaxWords), M);
    const uint32_t nchunks = (uint32_t)((M + C - 1) / C);
    RouteScratch& ws = r.route_ws;
    ws.use_on(st);
    ws.plane.reserve((uint64_t)idb * PW);
    ws.meta.reserve(2ull * PW + 1);
    ws.tr.reserve(idb);
    ws.scan.reserve(6ull * nchunks * PW);
    unsigned long long* any = ws.meta.p;
    unsigned long long* act = any + PW;
    unsigned long long* tany = act + PW;
    unsigned long long* agg = ws.scan.p;
    unsigned long long* carry = agg + 4ull * nchunks * PW;
    RP_HIP(hipMemsetAsync(ws.meta.p, 0, (2ull * PW + 1) * 8, st));
    hipLaunchKernelGGL(k_route_pack, dim3((idb + kRoutePackThreads - 1) / kRoutePackThreads, PW),
                       dim3(kRoutePackThreads), 0, st, rows, row_stride, bit, V, col, idb, r.d_inring.p, r.inring_n,
                       truth, active, PW, ws.plane.p, any, act, tany, ws.tr.p);
    RP_HIP(hipGetLastError());
    const RingView rv = r.view();
    constexpr uint32_t wpb = kShareThreads / 64;
    hipLaunchKernelGGL(k_share_reduce, dim3(nchunks, ((PW + 63u) / 64u + wpb - 1) / wpb), dim3(kShareThreads), 0, st,
                       rv.own, M, (uint32_t)C, ws.plane.p, ws.tr.p, PW, agg);
    RP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_share_carry, dim3((PW + kShareCarryThreads - 1) / kShareCarryThreads),
                       dim3(kShareCarryThreads), 0, st, agg, nchunks, PW, carry);
    RP_HIP(hipGetLastError());
    const dim3 grid(nchunks, (PW + wpb - 1) / wpb);
    if (pos_wrong)
        hipLaunchKernelGGL(k_share_apply<true>, grid, dim3(kShareThreads), 0, st, rv, (uint32_t)C, ws.plane.p, act,
                           ws.tr.p, carry, PW, reinterpret_cast<unsigned long long*>(wrong),
                           reinterpret_cast<unsigned long long*>(lost), pos_wrong);
    else
        hipLaunchKernelGGL(k_share_apply<false>, grid, dim3(kShareThreads), 0, st, rv, (uint32_t)C, ws.plane.p, act,
                           ws.tr.p, carry, PW, reinterpret_cast<unsigned long long*>(wrong),
                           reinterpret_cast<unsigned long long*>(lost), pos_wrong);
    RP_HIP(hipGetLastError());
}

}  // namespace rp

// ==================================================================================== C ABI

struct rp_ring {
    rp::Ring impl;
};
struct rp_ring_snap {
    rp::Snap impl;
};

using rp::guard;
using rp::guard_host;

namespace rp {
int ring_device(const rp_ring* h) { return h ? h->impl.device : -1; }  // (rp_sim_routing's device check)
}

static rp::Ring& R(rp_ring* r) {
    if (!r) throw rp::Error(rp::RP_EINVAL, "null ring handle");
    RP_HIP(hipSetDevice(r->impl.device));
    return r->impl;
}

// The caller's keys, as every batch entry point takes them: key bytes (stride > 0: key i is
// keys[i * stride .. + stride), else keys[off[i] .. off[i + 1])) or, from a caller hashFunc, the
// key hashes. `hashed` says which form the entry point is; its buffer may still be null.
struct KeySrc {
    const char* keys;
    const uint64_t* off;
    uint32_t stride;
    const uint32_t* hashes;
    bool hashed;
};
static KeySrc key_bytes(const void* keys, const uint64_t* off, uint32_t stride) {
    return {static_cast<const char*>(keys), off, stride, nullptr, false};
}
static KeySrc key_hashes(const uint32_t* hashes) { return {nullptr, nullptr, 0, hashes, true}; }

// RP_EINVAL "<op>: null key buffer" (or "null hash buffer") unless n == 0 or the source is all
// there. The lookups test their output buffer in the same breath (`rest`) and name no kind (`what`).
static void require_keys(const char* op, const KeySrc& k, uint64_t n, bool rest = true, const char* what = nullptr) {
    const bool given = k.hashed ? k.hashes != nullptr : (k.keys && (k.stride || k.off));
    if (n == 0 || (given && rest)) return;
    throw rp::Error(rp::RP_EINVAL, std::string(op) + ": null " + (what ? what : k.hashed ? "hash buffer" : "key buffer"));
}

// The host forms' staging, on r.st through the handle's buffers: hashes -> io_a; else the key
// bytes -> io_keys (with 16 bytes of tail for the kernels' wide loads) and, without a stride, the
// offsets -> io_off. n == 0 stages nothing. The pointers are what the rp:: passes take.
static rp::DevKeys stage_keys(rp::Ring& r, const KeySrc& k, uint64_t n) {
    rp::DevKeys d{nullptr, nullptr, k.stride, nullptr};
    if (n == 0) return d;
    if (k.hashed) {
        r.io_a.reserve(n);
        RP_HIP(hipMemcpyAsync(r.io_a.p, k.hashes, n * 4, hipMemcpyHostToDevice, r.st));
        d.hashes = r.io_a.p;
        return d;
    }
    const uint64_t bytes = k.stride ? n * k.stride : k.off[n];
    r.io_keys.reserve(bytes + 16);
    RP_HIP(hipMemcpyAsync(r.io_keys.p, k.keys, bytes, hipMemcpyHostToDevice, r.st));
    d.keys = r.io_keys.p;
    if (!k.stride) {
        r.io_off.reserve(n + 1);
        RP_HIP(hipMemcpyAsync(r.io_off.p, k.off, (n + 1) * 8, hipMemcpyHostToDevice, r.st));
        d.off = r.io_off.p;
    }
    return d;
}

// The routing host forms' views and per-view outputs, staged on r.st through the ring's route
// scratch: io8 = [rows V * row_stride | truth row_stride | active V], io32 = [col id bound | the
// caller's `extra` uint32 outputs (out32)], io64 = [wrong V | lost V], which hold the caller's
// values under accumulate. A null host buffer stays a null pointer. unstage_views queues the
// copies of wrong / lost back; the caller copies out32 and synchronizes.
struct DevViews {
    const uint8_t *rows, *truth, *active;
    const uint32_t* col;
    uint32_t* out32;
    uint64_t *wrong, *lost;
};
static DevViews stage_views(rp::Ring& r, const uint8_t* rows, uint64_t row_stride, uint64_t V, const uint32_t* col,
                            const uint8_t* truth, const uint8_t* active, int accumulate, const uint64_t* wrong,
                            const uint64_t* lost, uint64_t extra) {
    rp::RouteScratch& ws = r.route_ws;
    ws.use_on(r.st);
    const uint64_t idb = r.nt.size(), rb = V * row_stride;
    ws.io8.reserve(rb + row_stride + V + 1);
    uint8_t* drows = ws.io8.p;
    uint8_t* dtruth = truth ? drows + rb : nullptr;
    uint8_t* dact = active ? drows + rb + row_stride : nullptr;
    if (rb) RP_HIP(hipMemcpyAsync(drows, rows, rb, hipMemcpyHostToDevice, r.st));
    if (truth && row_stride) RP_HIP(hipMemcpyAsync(dtruth, truth, row_stride, hipMemcpyHostToDevice, r.st));
    if (active && V) RP_HIP(hipMemcpyAsync(dact, active, V, hipMemcpyHostToDevice, r.st));
    ws.io32.reserve(idb + extra + 1);
    uint32_t* dcol = col ? ws.io32.p : nullptr;
    if (col && idb) RP_HIP(hipMemcpyAsync(dcol, col, idb * 4, hipMemcpyHostToDevice, r.st));
    ws.io64.reserve(2 * V + 1);
    unsigned long long* dwr = wrong ? ws.io64.p : nullptr;
    unsigned long long* dlo = lost ? ws.io64.p + V : nullptr;
    if (accumulate && V) {
        if (wrong) RP_HIP(hipMemcpyAsync(dwr, wrong, V * 8, hipMemcpyHostToDevice, r.st));
        if (lost) RP_HIP(hipMemcpyAsync(dlo, lost, V * 8, hipMemcpyHostToDevice, r.st));
    }
    return {drows, dtruth, dact, dcol, ws.io32.p + idb, reinterpret_cast<uint64_t*>(dwr),
            reinterpret_cast<uint64_t*>(dlo)};
}
static void unstage_views(rp::Ring& r, const DevViews& dv, uint64_t V, uint64_t* wrong, uint64_t* lost) {
    if (V == 0) return;
    if (wrong) RP_HIP(hipMemcpyAsync(wrong, dv.wrong, V * 8, hipMemcpyDeviceToHost, r.st));
    if (lost) RP_HIP(hipMemcpyAsync(lost, dv.lost, V * 8, hipMemcpyDeviceToHost, r.st));
}

extern "C" {

int rp_ring_create(uint32_t replica_points, int device, rp_ring** out) {
    return guard([&] {
        RP_REQUIRE(out, "out is null");
        int nd = 0;
        RP_HIP(hipGetDeviceCount(&nd));
        RP_REQUIRE(device >= 0 && device < nd, "no such HIP device");
        RP_HIP(hipSetDevice(device));
        auto* h = new rp_ring();
        h->impl.device = device;
        h->impl.R = replica_points ? replica_points : 100;
        hipError_t e = hipStreamCreateWithFlags(&h->impl.st, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete h;
            throw rp::Error(rp::RP_EDEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
        }
        h->impl.tok.reserve(64);
        h->impl.own.reserve(64);
        rp::ring_rebuild_index(h->impl);
        *out = h;
    });
}

// ---- the lookup service (rp_ring_service; k_lookup_service)
// While the service wave is resident (up to idle_ms after a request), any hipFree in the process
// (a device buffer growing or released) synchronizes the device and so waits for the wave to idle
// out, and the wave's stream may share a hardware queue with another handle's. Every device call of
// the library therefore stops every resident service first and keeps new ones from starting while
// it runs (QuietScope, rp_common.h): rings with a service configured are listed
// in a process-wide registry that svc_quiesce walks.
}  // extern "C" (the registry and its counters have C++ linkage)
namespace rp {
std::atomic<int> g_quiet{0}, g_svc_live{0};
}  // namespace rp
static std::mutex g_svc_reg_mu;            // guards g_svc_reg; taken before any ring's svc_mu
static std::vector<rp::Ring*> g_svc_reg;   // rings with a service configured (rp_ring_service)

static void svc_stop(rp::Ring& r) {
    std::lock_guard<std::recursive_mutex> lk(r.svc_mu);
    if (r.svc_prof[8] && getenv("RP_SVC_PROF")) {
        const double n = (double)r.svc_prof[8];
        fprintf(stderr,
                "[rp] service: %llu calls; device us per call: poll round trip %.3f, lookup %.3f; "
                "direct table %llu, window %llu, exact walk %llu, wide walk %llu\n",
                (unsigned long long)r.svc_prof[8], r.svc_prof[0] / n / 100.0, r.svc_prof[1] / n / 100.0,
                (unsigned long long)r.svc_prof[4], (unsigned long long)r.svc_prof[5],
                (unsigned long long)r.svc_prof[6], (unsigned long long)r.svc_prof[7]);
        for (auto& x : r.svc_prof) x = 0;
    }
    if (!r.svc || !r.svc_live.load()) return;
    __atomic_store_n(&r.svc->req[4], 1u, __ATOMIC_RELEASE);
    const hipError_t e = hipStreamSynchronize(r.svc_st);
    r.svc_live.store(false);
    rp::g_svc_live.fetch_sub(1);
    __atomic_store_n(&r.svc->req[4], 0u, __ATOMIC_RELEASE);
    RP_HIP(e);
}

void rp::svc_quiesce(const void* keep) {
    std::lock_guard<std::mutex> g(g_svc_reg_mu);
    for (rp::Ring* r : g_svc_reg)
        if (r != keep && r->svc_live.load()) svc_stop(*r);
}

static void svc_register(rp::Ring& r, bool on) {
    std::lock_guard<std::mutex> g(g_svc_reg_mu);
    auto it = std::find(g_svc_reg.begin(), g_svc_reg.end(), &r);
    if (on && it == g_svc_reg.end()) g_svc_reg.push_back(&r);
    if (!on && it != g_svc_reg.end()) g_svc_reg.erase(it);
}
extern "C" {

static void svc_launch(rp::Ring& r, uint32_t last) {
    using namespace rp;
    const uint64_t idle = (uint64_t)r.svc_idle_ms * 100000ull, maxt = 30ull * 100000000ull;  // 100 MHz ticks
    const CompactFixView fv{r.tok.p, r.own.p, r.cidx.p, r.view(), r.M, r.ccb};
    if (r.svc_v2) {
        const uint32_t warm = (uint32_t)env_pos("RP_SVC_WARM", 0), prof = getenv("RP_SVC_PROF") ? 1u : 0u;
        if (!r.svc_dt_valid) {  // the direct table for this ring (A/B: RP_SVC_DT=0)
            r.svc_dtb = 0;
            uint32_t B = 16;
            while (B < 22 && (1ull << B) < r.M) B++;
            const bool dt_on = !(getenv("RP_SVC_DT") && !strcmp(getenv("RP_SVC_DT"), "0"));
            if (dt_on && r.M > 0 && (1ull << B) >= r.M && r.nt.size() < 0xFFFFu) {
                r.svc_dt.reserve(4ull << B);
                hipLaunchKernelGGL(k_dt_build, dim3(grid_for(1ull << B, 256, 1u << 20)), dim3(256), 0, r.svc_st, r.tok.p,
                                   r.own.p, r.M, B, r.svc_dt.p);
                RP_HIP(hipGetLastError());
                r.svc_dtb = B;
            }
            r.svc_dt_valid = true;
        }
        const uint32_t* dt = r.svc_dtb ? reinterpret_cast<const uint32_t*>(r.svc_dt.p) : nullptr;
        // RP_SVC_WAVES pollers (one workgroup each, so one an XCD up to 8): see k_lookup_service3
        const uint32_t waves = (uint32_t)std::min<uint64_t>(env_pos("RP_SVC_WAVES", kSvcWaves), 16);
        hipLaunchKernelGGL((k_lookup_service3<RingView>), dim3(waves), dim3(64), 0, r.svc_st, r.svc_dev, r.view(), fv,
                           r.cview(lookup_knobs()), r.compact ? 1u : 0u, last, idle, maxt, warm, prof, dt, r.svc_dtb,
                           waves > 1 ? (uint32_t)env_pos("RP_SVC_PERIOD", kSvcPeriod) : 0u,
                           (getenv("RP_SVC_ANS") && !strcmp(getenv("RP_SVC_ANS"), "0")) ? 1u : 0u);
    } else
        hipLaunchKernelGGL((k_lookup_service<RingView>), dim3(1), dim3(64), 0, r.svc_st, r.svc_dev, r.view(), fv,
                           r.compact ? 1u : 0u, last, idle, maxt);
    RP_HIP(hipGetLastError());
}

int rp_ring_destroy(rp_ring* r) {
    return guard([&] {
        if (!r) return;
        svc_register(r->impl, false);  // no quiesce walks this ring from here on
        (void)hipSetDevice(r->impl.device);
        if (r->impl.st) {
            (void)hipStreamSynchronize(r->impl.st);
            (void)hipStreamDestroy(r->impl.st);
        }
        if (r->impl.svc) {
            try {
                svc_stop(r->impl);
            } catch (...) {
            }
            (void)hipStreamDestroy(r->impl.svc_st);
            (void)hipHostFree(r->impl.svc);
        }
        if (r->impl.pin_out) (void)hipHostFree(r->impl.pin_out);
        if (r->impl.pin_cnt) (void)hipHostFree(r->impl.pin_cnt);
        delete r;
    });
}

int rp_ring_add_remove(rp_ring* h, const char* add_bytes, const uint32_t* add_off, uint32_t n_add,
                       const uint32_t* add_tokens, const char* rem_bytes, const uint32_t* rem_off, uint32_t n_rem,
                       const uint32_t* rem_tokens, int* changed_out) {
    return guard([&] {
        rp::Ring& r = R(h);
        RP_REQUIRE(n_add == 0 || (add_bytes && add_off), "add names missing");
        svc_stop(r);  // the service reads the table this rebuilds
        RP_REQUIRE(n_rem == 0 || (rem_bytes && rem_off), "remove names missing");
        // lib/ring/index.js:69-76 — adds in order, skipping servers already present
        std::vector<uint32_t> add_ids, rem_ids;
        std::vector<uint32_t> add_tok_sel, rem_tok_sel;
        for (uint32_t j = 0; j < n_add; j++) {
            const uint32_t id = rp::ring_intern(r, add_bytes + add_off[j], add_off[j + 1] - add_off[j]);
            if (r.in_ring[id]) continue;
            r.in_ring[id] = 1;
            r.stamp[id] = r.next_stamp++;
            r.server_count++;
            add_ids.push_back(id);
            if (add_tokens)
                add_tok_sel.insert(add_tok_sel.end(), add_tokens + (uint64_t)j * r.R,
                                   add_tokens + (uint64_t)(j + 1) * r.R);
        }
        // :78-85 — then removes in order, skipping absent servers
        for (uint32_t j = 0; j < n_rem; j++) {
            const uint32_t id = r.nt.find(rem_bytes + rem_off[j], rem_off[j + 1] - rem_off[j]);
            if (id == rp::NIL || !r.in_ring[id]) continue;
            r.in_ring[id] = 0;
            r.server_count--;
            rem_ids.push_back(id);
            if (rem_tokens)
                rem_tok_sel.insert(rem_tok_sel.end(), rem_tokens + (uint64_t)j * r.R,
                                   rem_tokens + (uint64_t)(j + 1) * r.R);
        }
        const bool changed = !add_ids.empty() || !rem_ids.empty();
        if (changed) {
            r.nt.sync(r.st);
            rp::ring_apply_adds(r, add_ids, add_tokens ? &add_tok_sel : nullptr);
            rp::ring_apply_removes(r, rem_ids, rem_tokens ? &rem_tok_sel : nullptr);
            rp::ring_rebuild_index(r);
            rp::ring_compute_checksum(r);  // (89-91)
            RP_HIP(hipStreamSynchronize(r.st));
        }
        if (changed_out) *changed_out = changed ? 1 : 0;
    });
}

int rp_ring_checksum(rp_ring* h, uint32_t* out, int* is_set) {
    return guard_host([&] {
        rp::Ring& r = R(h);
        if (out) *out = r.checksum;
        if (is_set) *is_set = r.has_checksum ? 1 : 0;
    });
}

int rp_ring_checksum_string(rp_ring* h, char* buf, uint64_t cap, uint64_t* len) {
    return guard([&] {
        rp::Ring& r = R(h);
        uint64_t L = 0;
        const uint32_t nn = r.nt.size();
        svc_stop(r);
        if (r.has_checksum && nn) {
            uint32_t total = 0;
            RP_HIP(hipMemcpyAsync(&total, r.pos.p + nn, 4, hipMemcpyDeviceToHost, r.st));
            RP_HIP(hipStreamSynchronize(r.st));
            L = total ? total - 1 : 0;
        }
        if (len) *len = L;
        const uint64_t n = std::min<uint64_t>(cap, L);
        if (buf && n) {
            RP_HIP(hipMemcpyAsync(buf, r.ck_buf.p, n, hipMemcpyDeviceToHost, r.st));
            RP_HIP(hipStreamSynchronize(r.st));
        }
    });
}

int rp_ring_server_count(rp_ring* h, uint32_t* out) {
    return guard_host([&] { *out = R(h).server_count; });
}

int rp_ring_token_count(rp_ring* h, uint32_t* out) {
    return guard_host([&] { *out = R(h).M; });
}

int rp_ring_has_server(rp_ring* h, const char* name, uint32_t len, int* out) {
    return guard_host([&] {
        rp::Ring& r = R(h);
        const uint32_t id = r.nt.find(name, len);
        *out = (id != rp::NIL && r.in_ring[id]) ? 1 : 0;
    });
}

int rp_ring_server_id(rp_ring* h, const char* name, uint32_t len, uint32_t* id) {
    return guard_host([&] {
        rp::Ring& r = R(h);
        *id = r.nt.find(name, len);
    });
}

const char* rp_ring_owner_name(rp_ring* h, uint32_t id, uint32_t* len) {
    if (!h || id >= h->impl.nt.size()) {
        if (len) *len = 0;
        return nullptr;
    }
    if (len) *len = (uint32_t)h->impl.nt.names[id].size();
    return h->impl.nt.names[id].data();
}

int rp_ring_servers(rp_ring* h, uint32_t* ids_out, uint32_t cap, uint32_t* n) {
    return guard_host([&] {
        rp::Ring& r = R(h);
        std::vector<uint32_t> v;
        for (uint32_t id = 0; id < r.nt.size(); id++)
            if (r.in_ring[id]) v.push_back(id);
        std::sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return r.stamp[a] < r.stamp[b]; });
        *n = (uint32_t)v.size();
        for (uint32_t i = 0; i < v.size() && i < cap; i++) ids_out[i] = v[i];
    });
}

int rp_ring_dump(rp_ring* h, uint32_t* tokens, uint32_t* owners, uint32_t cap) {
    return guard([&] {
        rp::Ring& r = R(h);
        const uint32_t n = std::min(cap, r.M);
        svc_stop(r);
        if (n) {
            if (tokens) RP_HIP(hipMemcpyAsync(tokens, r.tok.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, r.st));
            if (owners) RP_HIP(hipMemcpyAsync(owners, r.own.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, r.st));
        }
        RP_HIP(hipStreamSynchronize(r.st));
    });
}

// ---- lookups

int rp_ring_lookupn_dev(rp_ring* h, const uint8_t* d_keys, const uint64_t* d_off, uint32_t stride, uint64_t n,
                        int32_t nrep, uint32_t* d_owners, uint8_t* d_counts, void* stream) {
    return guard([&] {
        rp::Ring& r = R(h);
        require_keys("lookupn_dev", key_bytes(d_keys, d_off, stride), n, d_owners != nullptr, "buffer");
        svc_stop(r);
        const auto [np, W] = rp::replicas(nrep, r.server_count);
        rp::launch_lookupn(r, d_keys, d_off, stride, nullptr, n, np, W, d_owners, d_counts, rp::as_stream(stream));
    });
}

int rp_ring_lookup_dev(rp_ring* h, const uint8_t* d_keys, const uint64_t* d_off, uint32_t stride, uint64_t n,
                       uint32_t* d_owners, void* stream) {
    return guard([&] {
        rp::Ring& r = R(h);
        require_keys("lookup_dev", key_bytes(d_keys, d_off, stride), n, d_owners != nullptr, "buffer");
        svc_stop(r);
        // lookup (:145-154) == a one-step walk, independent of getServerCount
        rp::launch_lookupn(r, d_keys, d_off, stride, nullptr, n, 1, 1, d_owners, nullptr, rp::as_stream(stream));
    });
}

int rp_ring_lookupn_hashes_dev(rp_ring* h, const uint32_t* d_hashes, uint64_t n, int32_t nrep, uint32_t* d_owners,
                               uint8_t* d_counts, void* stream) {
    return guard([&] {
        rp::Ring& r = R(h);
        require_keys("lookupn_hashes_dev", key_hashes(d_hashes), n, d_owners != nullptr, "buffer");
        svc_stop(r);
        const auto [np, W] = rp::replicas(nrep, r.server_count);
        rp::launch_lookupn(r, nullptr, nullptr, 0, d_hashes, n, np, W, d_owners, d_counts, rp::as_stream(stream));
    });
}

// host-buffer forms: stage through the handle's device buffers on its stream
// The small path: at most kSmallKeys keys of kSmallBytes in all, rows of at most kSmallW owners,
// on the wide view (binary search + the reference walk). RP_RING_SMALL=0 turns it off (A/B).
static bool host_lookup_small(rp::Ring& r, const char* keys, const uint64_t* off, uint32_t stride, uint64_t n, int np,
                              uint32_t W, uint32_t* owners, uint8_t* counts) {
    using namespace rp;
    const char* se = getenv("RP_RING_SMALL");
    const bool on = !(se && !strcmp(se, "0"));
    const int need = np <= 0 ? 1 : np;
    if (!on || n > kSmallKeys || W > kSmallW || need > 8 || r.M == 0) return false;
    const uint64_t bytes = stride ? n * stride : off[n] - off[0];
    if (bytes > kSmallBytes) return false;
    SmallKeys sk;
    sk.n = (uint32_t)n;
    for (uint64_t k = 0; k <= n; k++) sk.off[k] = (uint16_t)(stride ? k * stride : off[k] - off[0]);
    memcpy(sk.b, keys + (stride ? 0 : off[0]), bytes);
    if (!r.pin_out) {
        RP_HIP(hipHostMalloc(reinterpret_cast<void**>(&r.pin_out), 4ull * kSmallKeys * kSmallW, hipHostMallocMapped));
        RP_HIP(hipHostMalloc(reinterpret_cast<void**>(&r.pin_cnt), kSmallKeys, hipHostMallocMapped));
        RP_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&r.pin_out_dev), r.pin_out, 0));
        RP_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&r.pin_cnt_dev), r.pin_cnt, 0));
    }
    const auto rv = r.view();
    uint8_t* cd = counts ? r.pin_cnt_dev : nullptr;
    if (need == 1)
        hipLaunchKernelGGL((k_lookupn_small<1, decltype(rv)>), dim3(1), dim3(64), 0, r.st, sk, rv, np, W, r.pin_out_dev, cd);
    else if (need <= 4)
        hipLaunchKernelGGL((k_lookupn_small<4, decltype(rv)>), dim3(1), dim3(64), 0, r.st, sk, rv, np, W, r.pin_out_dev, cd);
    else
        hipLaunchKernelGGL((k_lookupn_small<8, decltype(rv)>), dim3(1), dim3(64), 0, r.st, sk, rv, np, W, r.pin_out_dev, cd);
    RP_HIP(hipGetLastError());
    RP_HIP(hipStreamSynchronize(r.st));
    memcpy(owners, r.pin_out, 4ull * n * W);
    if (counts) memcpy(counts, r.pin_cnt, n);
    return true;
}

// one key (or, with hash non-null, one caller hash) through the service: false when it does not
// apply (off, a wide row; the round-4 kernel: a long key or a caller hash)
static bool svc_lookup(rp::Ring& r, const char* key, uint32_t len, const uint32_t* hash, int np, uint32_t W,
                       uint32_t* owners, uint8_t* counts) {
    using namespace rp;
    const int need = np <= 0 ? 1 : np;
    if (!r.svc_idle_ms || W > 8 || need > 8 || r.M == 0) return false;
    if (!r.svc_v2 && (hash || len > kSvcKeyMax)) return false;
    if (g_quiet.load() > 0) return false;  // another thread's device call is running
    if (g_svc_live.load() > (r.svc_live.load() ? 1 : 0)) rp::svc_quiesce(&r);  // another ring's wave
    std::lock_guard<std::recursive_mutex> lk(r.svc_mu);
    if (!r.svc) {
        RP_HIP(hipHostMalloc(reinterpret_cast<void**>(&r.svc), sizeof(SvcLines), hipHostMallocMapped | hipHostMallocCoherent));
        memset(r.svc, 0, sizeof(SvcLines));
        RP_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&r.svc_dev), r.svc, 0));
        RP_HIP(hipStreamCreateWithFlags(&r.svc_st, hipStreamNonBlocking));
        r.svc_seq = 0;
    }
    SvcLines* io = r.svc;
    // a wave is needed: none launched, or the last one exited (idle or lifetime). Announce it in
    // g_svc_live before reading g_quiet (the QuietScope handshake, rp_common.h); while another
    // thread's device call runs, this lookup takes the launch path instead.
    bool launch = false;
    if (!r.svc_live.load()) {
        r.svc_live.store(true);
        g_svc_live.fetch_add(1);
        if (g_quiet.load() > 0) {
            r.svc_live.store(false);
            g_svc_live.fetch_sub(1);
            return false;
        }
        launch = true;
    } else if (hipStreamQuery(r.svc_st) == hipSuccess) {
        launch = true;
    }
    const uint32_t s = r.svc_seq + 1;
    if (r.svc_v2) {
        // the key's hash, on the host as the reference computes it (lib/ring/index.js:145-154)
        io->req[1] = hash ? *hash : fh::hash32(fh::PtrSrc{reinterpret_cast<const uint8_t*>(key)}, len);
    } else {
        for (uint32_t c = 0; c * 60 < len; c++) {  // each key line's bytes, then its seq
            memcpy(&io->req[16 * (c + 1)], key + 60 * c, std::min<uint32_t>(60, len - 60 * c));
            __atomic_store_n(&io->req[16 * (c + 1) + 15], s, __ATOMIC_RELEASE);
        }
        io->req[1] = len;
    }
    io->req[2] = (uint32_t)np;
    io->req[3] = W;
    __atomic_store_n(&io->req[15], s, __ATOMIC_RELEASE);  // the header's trailing copy of seq
    __atomic_store_n(&io->req[0], s, __ATOMIC_RELEASE);
    if (launch) svc_launch(r, s - 1);
    uint64_t spins = 0;
    const auto t0 = std::chrono::steady_clock::now();
    // v2: the answer line is taken when all 8 of its words carry seq s (no torn line)
    auto answered = [&]() -> bool {
        if (!r.svc_v2) return __atomic_load_n(&io->resp_seq[0], __ATOMIC_ACQUIRE) == s;
        const uint64_t* a = io->resp2[s & 7u];
        if ((uint32_t)(__atomic_load_n(&a[7], __ATOMIC_ACQUIRE) >> 32) != s) return false;
        for (int q = 0; q < 7; q++)
            if ((uint32_t)(__atomic_load_n(&a[q], __ATOMIC_ACQUIRE) >> 32) != s) return false;
        return true;
    };
    while (!answered()) {
        __builtin_ia32_pause();
        if ((++spins & 4095) == 0) {
            if (hipStreamQuery(r.svc_st) == hipSuccess && !answered()) {
                svc_launch(r, s - 1);  // it exited (idle or lifetime) before taking this request
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
                svc_stop(r);
                throw Error(RP_EDEVICE, "lookup service: no answer within 5 s");
            }
        }
    }
    r.svc_seq = s;
    if (r.svc_v2 && getenv("RP_SVC_PROF") && __atomic_load_n(&io->diag[0], __ATOMIC_ACQUIRE) == s) {
        r.svc_prof[0] += io->diag[1];
        r.svc_prof[1] += io->diag[2];
        r.svc_prof[4 + (io->diag[3] & 3)]++;
        r.svc_prof[8]++;
    }
    if (r.svc_v2) {
        uint32_t c = 0;
        for (uint32_t q = 0; q < W; q++) {
            owners[q] = (uint32_t)io->resp2[s & 7u][q];
            c += (c == q && owners[q] != NIL) ? 1u : 0u;
        }
        if (counts) counts[0] = (uint8_t)c;
        return true;
    }
    for (uint32_t q = 0; q < W; q++) owners[q] = io->resp[q];
    if (counts) counts[0] = (uint8_t)io->resp[15];
    return true;
}

static void host_lookup(rp::Ring& r, const KeySrc& k, uint64_t n, int np, uint32_t W, uint32_t* owners,
                        uint8_t* counts) {
    if (n == 0) return;
    if (n == 1 && (k.hashed ? svc_lookup(r, nullptr, 0, k.hashes, np, W, owners, counts)
                            : svc_lookup(r, k.keys + (k.stride ? 0 : k.off[0]),
                                         (uint32_t)(k.stride ? k.stride : k.off[1] - k.off[0]), nullptr, np, W, owners,
                                         counts)))
        return;
    rp::QuietScope quiet;  // the launch path: no resident service (this ring's or another's) meanwhile
    svc_stop(r);
    if (!k.hashed && host_lookup_small(r, k.keys, k.off, k.stride, n, np, W, owners, counts)) return;
    const rp::DevKeys d = stage_keys(r, k, n);
    r.io_b.reserve(n * W);
    if (counts) r.io_cnt.reserve(n);
    rp::launch_lookupn(r, d.keys, d.off, d.stride, d.hashes, n, np, W, r.io_b.p, counts ? r.io_cnt.p : nullptr, r.st);
    RP_HIP(hipMemcpyAsync(owners, r.io_b.p, n * W * 4, hipMemcpyDeviceToHost, r.st));
    if (counts) RP_HIP(hipMemcpyAsync(counts, r.io_cnt.p, n, hipMemcpyDeviceToHost, r.st));
    RP_HIP(hipStreamSynchronize(r.st));
}

int rp_ring_service(rp_ring* h, uint32_t idle_ms) {
    return guard([&] {
        rp::Ring& r = R(h);
        svc_stop(r);
        svc_register(r, idle_ms > 0);
        r.svc_idle_ms = idle_ms;
        r.svc_v2 = !(getenv("RP_RING_SVC") && !strcmp(getenv("RP_RING_SVC"), "1"));
    });
}

int rp_ring_lookup(rp_ring* h, const char* keys, const uint64_t* off, uint32_t stride, uint64_t n, uint32_t* owners) {
    return guard_host([&] {
        rp::Ring& r = R(h);
        const KeySrc k = key_bytes(keys, off, stride);
        require_keys("lookup", k, n, owners != nullptr, "buffer");
        host_lookup(r, k, n, 1, 1, owners, nullptr);
    });
}

int rp_ring_lookupn(rp_ring* h, const char* keys, const uint64_t* off, uint32_t stride, uint64_t n, int32_t nrep,
                    uint32_t* owners, uint8_t* counts) {
    return guard_host([&] {
        rp::Ring& r = R(h);
        const KeySrc k = key_bytes(keys, off, stride);
        require_keys("lookupn", k, n, owners != nullptr, "buffer");
        const auto [np, W] = rp::replicas(nrep, r.server_count);
        host_lookup(r, k, n, np, W, owners, counts);
    });
}

int rp_ring_lookup_hashes(rp_ring* h, const uint32_t* hashes, uint64_t n, uint32_t* owners) {
    return guard_host([&] {
        rp::Ring& r = R(h);
        const KeySrc k = key_hashes(hashes);
        require_keys("lookup_hashes", k, n, owners != nullptr, "buffer");
        host_lookup(r, k, n, 1, 1, owners, nullptr);
    });
}

int rp_ring_lookupn_hashes(rp_ring* h, const uint32_t* hashes, uint64_t n, int32_t nrep, uint32_t* owners,
                           uint8_t* counts) {
    return guard_host([&] {
        rp::Ring& r = R(h);
        const KeySrc k = key_hashes(hashes);
        require_keys("lookupn_hashes", k, n, owners != nullptr, "buffer");
        const auto [np, W] = rp::replicas(nrep, r.server_count);
        host_lookup(r, k, n, np, W, owners, counts);
    });
}

// ---- group keys by owner (handleOrProxyAll / lookupKeys)

int rp_ring_group_keys_dev(rp_ring* h, const uint8_t* d_keys, const uint64_t* d_off, uint32_t stride, uint64_t n,
                           uint32_t self_id, uint32_t* d_dests, uint32_t* d_group_off, uint32_t* d_perm,
                           uint32_t* d_ndest, void* stream) {
    return guard([&] {
        rp::Ring& r = R(h);
        RP_REQUIRE(d_dests && d_group_off && d_perm && d_ndest, "group_keys_dev: null output buffer");
        require_keys("group_keys_dev", key_bytes(d_keys, d_off, stride), n);
        svc_stop(r);
        rp::group_keys(r, d_keys, d_off, stride, nullptr, n, self_id, d_dests, d_group_off, d_perm, d_ndest,
                       rp::as_stream(stream));
    });
}

// host-buffer forms: keys (or a caller hashFunc's key hashes) in, groups out
static void host_group(rp::Ring& r, const KeySrc& k, uint64_t n, uint32_t self_id, uint32_t* dests, uint32_t* goff,
                       uint32_t* perm, uint32_t* ndest) {
    RP_REQUIRE(dests && goff && perm && ndest, "group_keys: null output buffer");
    svc_stop(r);
    const rp::DevKeys d = stage_keys(r, k, n);
    // io_b = [perm n | group_off n+1 | dests n | ndest 1]
    const uint64_t nn = n ? n : 1;
    r.io_b.reserve(3 * nn + 2);
    uint32_t* dperm = r.io_b.p;
    uint32_t* dgoff = dperm + nn;
    uint32_t* ddest = dgoff + nn + 1;
    uint32_t* dnd = ddest + nn;
    rp::group_keys(r, d.keys, d.off, d.stride, d.hashes, n, self_id, ddest, dgoff, dperm, dnd, r.st);
    uint32_t nd = 0;
    RP_HIP(hipMemcpyAsync(&nd, dnd, 4, hipMemcpyDeviceToHost, r.st));
    RP_HIP(hipStreamSynchronize(r.st));
    *ndest = nd;
    if (n) RP_HIP(hipMemcpyAsync(perm, dperm, n * 4, hipMemcpyDeviceToHost, r.st));
    if (nd) RP_HIP(hipMemcpyAsync(dests, ddest, 4ull * nd, hipMemcpyDeviceToHost, r.st));
    RP_HIP(hipMemcpyAsync(goff, dgoff, 4ull * (nd + 1), hipMemcpyDeviceToHost, r.st));
    RP_HIP(hipStreamSynchronize(r.st));
}

int rp_ring_group_keys(rp_ring* h, const char* keys, const uint64_t* off, uint32_t stride, uint64_t n,
                       uint32_t self_id, uint32_t* dests, uint32_t* group_off, uint32_t* perm, uint32_t* ndest) {
    return guard([&] {
        rp::Ring& r = R(h);
        const KeySrc k = key_bytes(keys, off, stride);
        require_keys("group_keys", k, n);
        host_group(r, k, n, self_id, dests, group_off, perm, ndest);
    });
}

int rp_ring_group_hashes(rp_ring* h, const uint32_t* hashes, uint64_t n, uint32_t self_id, uint32_t* dests,
                         uint32_t* group_off, uint32_t* perm, uint32_t* ndest) {
    return guard([&] {
        rp::Ring& r = R(h);
        const KeySrc k = key_hashes(hashes);
        require_keys("group_hashes", k, n);
        host_group(r, k, n, self_id, dests, group_off, perm, ndest);
    });
}

// ---- ring snapshots and moved keys

int rp_ring_snapshot(rp_ring* h, rp_ring_snap** out) {
    return guard([&] {
        rp::Ring& r = R(h);
        RP_REQUIRE(out, "snapshot: out is null");
        svc_stop(r);
        std::unique_ptr<rp_ring_snap> s(new rp_ring_snap());
        rp::Snap& d = s->impl;
        d.device = r.device;
        d.M = r.M;
        d.bbits = r.bbits;
        d.server_count = r.server_count;
        d.id_bound = r.nt.size();
        d.checksum = r.checksum;
        d.has_checksum = r.has_checksum;
        const uint64_t nbk = (1ull << r.bbits) + 1;
        d.tok.reserve(r.M);
        d.own.reserve(r.M);
        d.bstart.reserve(nbk);
        if (r.M) {
            RP_HIP(hipMemcpyAsync(d.tok.p, r.tok.p, 4ull * r.M, hipMemcpyDeviceToDevice, r.st));
            RP_HIP(hipMemcpyAsync(d.own.p, r.own.p, 4ull * r.M, hipMemcpyDeviceToDevice, r.st));
        }
        RP_HIP(hipMemcpyAsync(d.bstart.p, r.bstart.p, 4ull * nbk, hipMemcpyDeviceToDevice, r.st));
        RP_HIP(hipStreamSynchronize(r.st));  // complete before any later rebuild or any caller stream reads it
        *out = s.release();
    });
}

int rp_ring_snap_destroy(rp_ring_snap* s) {
    return guard([&] {  // (the buffers' hipFree synchronizes the device: no resident service meanwhile)
        if (!s) return;
        (void)hipSetDevice(s->impl.device);
        delete s;
    });
}

int rp_ring_snap_info(const rp_ring_snap* s, uint32_t* token_count, uint32_t* server_count, uint32_t* checksum,
                      int* checksum_is_set) {
    return guard_host([&] {
        RP_REQUIRE(s, "null snapshot handle");
        if (token_count) *token_count = s->impl.M;
        if (server_count) *server_count = s->impl.server_count;
        if (checksum) *checksum = s->impl.checksum;
        if (checksum_is_set) *checksum_is_set = s->impl.has_checksum ? 1 : 0;
    });
}

int rp_ring_snap_lookupn_dev(rp_ring_snap* s, const uint8_t* d_keys, const uint64_t* d_off, uint32_t stride,
                             uint64_t n, int32_t nrep, uint32_t* d_owners, uint8_t* d_counts, void* stream) {
    return guard([&] {
        RP_REQUIRE(s, "null snapshot handle");
        require_keys("snap_lookupn_dev", key_bytes(d_keys, d_off, stride), n, d_owners != nullptr, "buffer");
        if (n == 0) return;
        RP_HIP(hipSetDevice(s->impl.device));
        const auto [np, W] = rp::replicas(nrep, s->impl.server_count);
        rp::launch_lookupn_view(s->impl.view(), d_keys, d_off, stride, nullptr, n, np, W, d_owners, d_counts,
                                rp::as_stream(stream), rp::lookup_knobs().ablate);
    });
}

static const rp::Snap& S(const rp_ring_snap* s) {
    if (!s) throw rp::Error(rp::RP_EINVAL, "null snapshot handle");
    return s->impl;
}

int rp_ring_moved_keys_dev(rp_ring* h, const rp_ring_snap* before, const uint8_t* d_keys, const uint64_t* d_off,
                           uint32_t stride, uint64_t n, int32_t nrep, uint32_t cap, uint32_t* d_idx,
                           uint32_t* d_before, uint32_t* d_after, uint32_t* d_count, void* stream) {
    return guard([&] {
        rp::Ring& r = R(h);
        const rp::Snap& s = S(before);
        require_keys("moved_keys_dev", key_bytes(d_keys, d_off, stride), n);
        svc_stop(r);
        rp::moved_keys(r, s, {d_keys, d_off, stride, nullptr}, n, nrep, cap, d_idx, d_before, d_after, d_count,
                       rp::as_stream(stream));
    });
}

// host-buffer forms: keys (or a caller hashFunc's key hashes) in, the moved list out
static void host_moved(rp::Ring& r, const rp::Snap& s, const KeySrc& k, uint64_t n, int32_t nrep, uint32_t cap,
                       uint32_t* idx, uint32_t* brows, uint32_t* arows, uint32_t* count) {
    RP_REQUIRE(count, "moved_keys: null count");
    RP_REQUIRE(nrep <= 8, "moved_keys: nrep is at most 8 (the rows are compared in registers)");
    RP_REQUIRE(n < (1ull << 32), "moved_keys: at most 2^32-1 keys per call");
    RP_REQUIRE(cap == 0 || n == 0 || idx, "moved_keys: null index buffer");
    svc_stop(r);
    const rp::DevKeys d = stage_keys(r, k, n);
    // io_b = [count 1 | idx c | before rows c*W | after rows c*W], c = min(cap, n)
    const uint64_t c = std::min<uint64_t>(cap, n), W = rp::replicas(nrep, r.server_count).W;
    r.io_b.reserve(1 + c * (1 + 2 * W));
    uint32_t* dcount = r.io_b.p;
    uint32_t* didx = dcount + 1;
    uint32_t* dbr = didx + c;
    uint32_t* dar = dbr + c * W;
    rp::moved_keys(r, s, d, n, nrep, (uint32_t)c, c ? didx : nullptr, brows ? dbr : nullptr,
                   arows ? dar : nullptr, dcount, r.st);
    uint32_t total = 0;
    RP_HIP(hipMemcpyAsync(&total, dcount, 4, hipMemcpyDeviceToHost, r.st));
    RP_HIP(hipStreamSynchronize(r.st));
    rp::scratch_check(r.ws, r.st);  // a look-back wait that gave up is an error, not a wrong list
    *count = total;
    const uint64_t m = std::min<uint64_t>(total, c);
    if (m) {
        RP_HIP(hipMemcpyAsync(idx, didx, m * 4, hipMemcpyDeviceToHost, r.st));
        if (brows) RP_HIP(hipMemcpyAsync(brows, dbr, m * W * 4, hipMemcpyDeviceToHost, r.st));
        if (arows) RP_HIP(hipMemcpyAsync(arows, dar, m * W * 4, hipMemcpyDeviceToHost, r.st));
        RP_HIP(hipStreamSynchronize(r.st));
    }
}

int rp_ring_moved_keys(rp_ring* h, const rp_ring_snap* before, const char* keys, const uint64_t* off, uint32_t stride,
                       uint64_t n, int32_t nrep, uint32_t cap, uint32_t* idx, uint32_t* before_rows,
                       uint32_t* after_rows, uint32_t* count) {
    return guard([&] {
        rp::Ring& r = R(h);
        const rp::Snap& s = S(before);
        const KeySrc k = key_bytes(keys, off, stride);
        require_keys("moved_keys", k, n);
        host_moved(r, s, k, n, nrep, cap, idx, before_rows, after_rows, count);
    });
}

int rp_ring_moved_hashes(rp_ring* h, const rp_ring_snap* before, const uint32_t* hashes, uint64_t n, int32_t nrep,
                         uint32_t cap, uint32_t* idx, uint32_t* before_rows, uint32_t* after_rows, uint32_t* count) {
    return guard([&] {
        rp::Ring& r = R(h);
        const rp::Snap& s = S(before);
        const KeySrc k = key_hashes(hashes);
        require_keys("moved_hashes", k, n);
        host_moved(r, s, k, n, nrep, cap, idx, before_rows, after_rows, count);
    });
}

// ---- hand-off plan

int rp_ring_handoff_dev(rp_ring* h, const rp_ring_snap* before, const uint8_t* d_keys, const uint64_t* d_off,
                        uint32_t stride, uint64_t n, int32_t nrep, uint32_t only_src, uint32_t cap, uint32_t* d_dests,
                        uint32_t* d_group_off, uint32_t* d_key_idx, uint32_t* d_src, uint8_t* d_slot,
                        uint32_t* d_ndest, uint32_t* d_count, void* stream) {
    return guard([&] {
        rp::Ring& r = R(h);
        const rp::Snap& s = S(before);
        require_keys("handoff_dev", key_bytes(d_keys, d_off, stride), n);
        svc_stop(r);
        rp::handoff(r, s, {d_keys, d_off, stride, nullptr}, n, nrep, only_src, cap, d_dests, d_group_off, d_key_idx,
                    d_src, d_slot, d_ndest, d_count, rp::as_stream(stream), false);
    });
}

// host-buffer forms: keys (or a caller hashFunc's key hashes) in, the grouped plan out
static void host_handoff(rp::Ring& r, const rp::Snap& s, const KeySrc& k, uint64_t n, int32_t nrep, uint32_t only_src,
                         uint32_t cap, uint32_t* dests, uint32_t* goff, uint32_t* key_idx, uint32_t* src,
                         uint8_t* slot, uint32_t* ndest, uint32_t* count) {
    const uint64_t W = rp::replicas(nrep, r.server_count).W;
    RP_REQUIRE(ndest && count, "handoff: null count");
    RP_REQUIRE(nrep <= 8, "handoff: nrep is at most 8 (the rows are compared in registers)");
    RP_REQUIRE(n < (1ull << 32) && n * W < (1ull << 32), "handoff: n * max(nrep, 1) is at most 2^32-1 records");
    RP_REQUIRE(s.device == r.device, "handoff: the snapshot lives on another device");
    RP_REQUIRE(only_src == rp::NIL || only_src < r.nt.size(), "handoff: only_src is not a server id of this ring");
    RP_REQUIRE(cap == 0 || n == 0 || (dests && goff && key_idx), "handoff: null output buffer");
    svc_stop(r);
    const rp::DevKeys d = stage_keys(r, k, n);
    // io = [count 1 | ndest 1 | group_off nd+1 | dests nd | key_idx c | src c | slot c bytes],
    // c = min(cap, n * W), nd = min(c, id bound)
    const uint64_t c = std::min<uint64_t>(cap, n * W), nd = std::min<uint64_t>(c, r.nt.size());
    rp::HandoffScratch& ws = r.handoff_ws;
    ws.use_on(r.st);
    ws.io.reserve(3 + 2 * nd + 2 * c + (c + 3) / 4);
    uint32_t* dgo = ws.io.p + 2;
    uint32_t* dde = dgo + nd + 1;
    uint32_t* dki = dde + nd;
    uint32_t* dsr = dki + c;
    uint8_t* dsl = reinterpret_cast<uint8_t*>(dsr + c);
    rp::handoff(r, s, d, n, nrep, only_src, (uint32_t)c, dde, dgo, dki, dsr, dsl,
                ws.io.p + 1, ws.io.p, r.st, true);
    uint32_t head[2] = {0, 0};
    RP_HIP(hipMemcpyAsync(head, ws.io.p, sizeof head, hipMemcpyDeviceToHost, r.st));
    RP_HIP(hipStreamSynchronize(r.st));
    rp::scratch_check(r.ws, r.st);
    *count = head[0];
    *ndest = head[1];
    const uint64_t T = std::min<uint64_t>(head[0], c), g = head[1];
    if (goff) RP_HIP(hipMemcpyAsync(goff, dgo, (g + 1) * 4, hipMemcpyDeviceToHost, r.st));
    if (T) {
        RP_HIP(hipMemcpyAsync(dests, dde, g * 4, hipMemcpyDeviceToHost, r.st));
        RP_HIP(hipMemcpyAsync(key_idx, dki, T * 4, hipMemcpyDeviceToHost, r.st));
        if (src) RP_HIP(hipMemcpyAsync(src, dsr, T * 4, hipMemcpyDeviceToHost, r.st));
        if (slot) RP_HIP(hipMemcpyAsync(slot, dsl, T, hipMemcpyDeviceToHost, r.st));
    }
    RP_HIP(hipStreamSynchronize(r.st));
}

int rp_ring_handoff(rp_ring* h, const rp_ring_snap* before, const char* keys, const uint64_t* off, uint32_t stride,
                    uint64_t n, int32_t nrep, uint32_t only_src, uint32_t cap, uint32_t* dests, uint32_t* group_off,
                    uint32_t* key_idx, uint32_t* src, uint8_t* slot, uint32_t* ndest, uint32_t* count) {
    return guard([&] {
        rp::Ring& r = R(h);
        const rp::Snap& s = S(before);
        const KeySrc k = key_bytes(keys, off, stride);
        require_keys("handoff", k, n);
        host_handoff(r, s, k, n, nrep, only_src, cap, dests, group_off, key_idx, src, slot, ndest, count);
    });
}

int rp_ring_handoff_hashes(rp_ring* h, const rp_ring_snap* before, const uint32_t* hashes, uint64_t n, int32_t nrep,
                           uint32_t only_src, uint32_t cap, uint32_t* dests, uint32_t* group_off, uint32_t* key_idx,
                           uint32_t* src, uint8_t* slot, uint32_t* ndest, uint32_t* count) {
    return guard([&] {
        rp::Ring& r = R(h);
        const rp::Snap& s = S(before);
        const KeySrc k = key_hashes(hashes);
        require_keys("handoff_hashes", k, n);
        host_handoff(r, s, k, n, nrep, only_src, cap, dests, group_off, key_idx, src, slot, ndest, count);
    });
}

// ---- routing agreement

int rp_ring_route_views_dev(rp_ring* h, const uint8_t* d_keys, const uint64_t* d_off, uint32_t stride,
                            const uint32_t* d_hashes, uint64_t n, const uint8_t* d_rows, uint64_t row_stride,
                            uint8_t bit, uint32_t n_views, const uint32_t* d_col, uint32_t id_cap,
                            const uint8_t* d_truth, const uint8_t* d_active, int accumulate, uint64_t* d_wrong,
                            uint64_t* d_lost, uint32_t* d_key_wrong, uint32_t* d_truth_owner, uint32_t* d_owners,
                            void* stream) {
    return guard([&] {
        rp::Ring& r = R(h);
        svc_stop(r);
        rp::route_views(r, {d_keys, d_off, stride, d_hashes}, n, d_rows, row_stride, bit, n_views, d_col, id_cap,
                        d_truth, d_active, accumulate, d_wrong, d_lost, d_key_wrong, d_truth_owner, d_owners,
                        rp::as_stream(stream));
    });
}

int rp_ring_route_views(rp_ring* h, const char* keys, const uint64_t* off, uint32_t stride, const uint32_t* hashes,
                        uint64_t n, const uint8_t* rows, uint64_t row_stride, uint8_t bit, uint32_t n_views,
                        const uint32_t* col, uint32_t id_cap, const uint8_t* truth, const uint8_t* active,
                        int accumulate, uint64_t* wrong, uint64_t* lost, uint32_t* key_wrong, uint32_t* truth_owner,
                        uint32_t* owners) {
    return guard([&] {
        rp::Ring& r = R(h);
        const uint64_t V = n_views, idb = r.nt.size();
        RP_REQUIRE(id_cap >= idb, "route_views: id_cap is below the ring's id bound (rp_ring_id_bound)");
        RP_REQUIRE(n == 0 || ((keys != nullptr) != (hashes != nullptr)),
                   "route_views: exactly one of the key buffer and the hash buffer");
        RP_REQUIRE(n == 0 || hashes || stride || off, "route_views: null key offsets");
        RP_REQUIRE(V == 0 || rows, "route_views: null view rows");
        svc_stop(r);
        const rp::DevKeys d = stage_keys(r, hashes ? key_hashes(hashes) : key_bytes(keys, off, stride), n);
        // the uint32 outputs: [key_wrong n | truth_owner n | owners n * V]
        const DevViews dv = stage_views(r, rows, row_stride, V, col, truth, active, accumulate, wrong, lost,
                                        2 * n + n * V);
        uint32_t* dkw = key_wrong ? dv.out32 : nullptr;
        uint32_t* dto = truth_owner ? dv.out32 + n : nullptr;
        uint32_t* dow = owners ? dv.out32 + 2 * n : nullptr;
        rp::route_views(r, d, n, dv.rows, row_stride, bit, n_views, dv.col, id_cap, dv.truth,
                        dv.active, accumulate, dv.wrong, dv.lost, dkw, dto, dow, r.st);
        unstage_views(r, dv, V, wrong, lost);
        if (n) {
            if (key_wrong) RP_HIP(hipMemcpyAsync(key_wrong, dkw, n * 4, hipMemcpyDeviceToHost, r.st));
            if (truth_owner) RP_HIP(hipMemcpyAsync(truth_owner, dto, n * 4, hipMemcpyDeviceToHost, r.st));
            if (owners && V) RP_HIP(hipMemcpyAsync(owners, dow, n * V * 4, hipMemcpyDeviceToHost, r.st));
        }
        RP_HIP(hipStreamSynchronize(r.st));
    });
}

int rp_ring_route_share_dev(rp_ring* h, const uint8_t* d_rows, uint64_t row_stride, uint8_t bit, uint32_t n_views,
                            const uint32_t* d_col, uint32_t id_cap, const uint8_t* d_truth, const uint8_t* d_active,
                            int accumulate, uint64_t* d_wrong, uint64_t* d_lost, uint32_t* d_pos_wrong,
                            uint32_t pos_cap, void* stream) {
    return guard([&] {
        rp::Ring& r = R(h);
        svc_stop(r);
        rp::route_share(r, d_rows, row_stride, bit, n_views, d_col, id_cap, d_truth, d_active, accumulate, d_wrong,
                        d_lost, d_pos_wrong, pos_cap, rp::as_stream(stream));
    });
}

int rp_ring_route_share(rp_ring* h, const uint8_t* rows, uint64_t row_stride, uint8_t bit, uint32_t n_views,
                        const uint32_t* col, uint32_t id_cap, const uint8_t* truth, const uint8_t* active,
                        int accumulate, uint64_t* wrong, uint64_t* lost, uint32_t* pos_wrong, uint32_t pos_cap) {
    return guard([&] {
        rp::Ring& r = R(h);
        const uint64_t V = n_views, M = r.M;
        RP_REQUIRE(id_cap >= r.nt.size(), "route_share: id_cap is below the ring's id bound (rp_ring_id_bound)");
        RP_REQUIRE(V == 0 || rows, "route_share: null view rows");
        RP_REQUIRE(!pos_wrong || pos_cap >= M, "route_share: pos_cap is below the token count");
        svc_stop(r);
        const DevViews dv = stage_views(r, rows, row_stride, V, col, truth, active, accumulate, wrong, lost, M);
        rp::route_share(r, dv.rows, row_stride, bit, n_views, dv.col, id_cap, dv.truth, dv.active, accumulate, dv.wrong,
                        dv.lost, pos_wrong ? dv.out32 : nullptr, pos_cap, r.st);
        unstage_views(r, dv, V, wrong, lost);
        if (pos_wrong && M) RP_HIP(hipMemcpyAsync(pos_wrong, dv.out32, M * 4, hipMemcpyDeviceToHost, r.st));
        RP_HIP(hipStreamSynchronize(r.st));
    });
}

// ---- owner load and hash-space share

int rp_ring_id_bound(rp_ring* h, uint32_t* out) {
    return guard_host([&] {
        rp::Ring& r = R(h);
        RP_REQUIRE(out, "id_bound: out is null");
        *out = r.nt.size();
    });
}

int rp_ring_owner_load_dev(rp_ring* h, const uint8_t* d_keys, const uint64_t* d_off, uint32_t stride, uint64_t n,
                           int32_t nrep, uint32_t id_cap, int accumulate, uint64_t* d_load, void* stream) {
    return guard([&] {
        rp::Ring& r = R(h);
        require_keys("owner_load_dev", key_bytes(d_keys, d_off, stride), n);
        svc_stop(r);
        rp::owner_load(r, r.load_ws, {d_keys, d_off, stride, nullptr}, n, nrep, id_cap, accumulate,
                       reinterpret_cast<unsigned long long*>(d_load), rp::as_stream(stream));
    });
}

// host-buffer forms: keys (or a caller hashFunc's key hashes) in, the counters out
static void host_owner_load(rp::Ring& r, const KeySrc& k, uint64_t n, int32_t nrep, uint32_t id_cap, uint64_t* load) {
    RP_REQUIRE(id_cap >= r.nt.size(), "owner_load: id_cap is below the ring's id bound (rp_ring_id_bound)");
    RP_REQUIRE(id_cap == 0 || load, "owner_load: null load buffer");
    svc_stop(r);
    const uint64_t bins = (uint64_t)id_cap * rp::replicas(nrep, r.server_count).W;
    if (bins == 0) return;
    const rp::DevKeys d = stage_keys(r, k, n);
    r.load_ws.use_on(r.st);
    r.load_ws.out.reserve(bins);
    rp::owner_load(r, r.load_ws, d, n, nrep, id_cap, 0, r.load_ws.out.p, r.st);
    RP_HIP(hipMemcpyAsync(load, r.load_ws.out.p, bins * sizeof(uint64_t), hipMemcpyDeviceToHost, r.st));
    RP_HIP(hipStreamSynchronize(r.st));
}

int rp_ring_owner_load(rp_ring* h, const char* keys, const uint64_t* off, uint32_t stride, uint64_t n, int32_t nrep,
                       uint32_t id_cap, uint64_t* load) {
    return guard([&] {
        rp::Ring& r = R(h);
        const KeySrc k = key_bytes(keys, off, stride);
        require_keys("owner_load", k, n);
        host_owner_load(r, k, n, nrep, id_cap, load);
    });
}

int rp_ring_owner_load_hashes(rp_ring* h, const uint32_t* hashes, uint64_t n, int32_t nrep, uint32_t id_cap,
                              uint64_t* load) {
    return guard([&] {
        rp::Ring& r = R(h);
        const KeySrc k = key_hashes(hashes);
        require_keys("owner_load_hashes", k, n);
        host_owner_load(r, k, n, nrep, id_cap, load);
    });
}

int rp_ring_snap_owner_load_dev(rp_ring_snap* s, const uint8_t* d_keys, const uint64_t* d_off, uint32_t stride,
                                uint64_t n, int32_t nrep, uint32_t id_cap, int accumulate, uint64_t* d_load,
                                void* stream) {
    return guard([&] {
        RP_REQUIRE(s, "null snapshot handle");
        require_keys("snap_owner_load_dev", key_bytes(d_keys, d_off, stride), n);
        rp::Snap& d = s->impl;
        RP_HIP(hipSetDevice(d.device));
        const rp::Replicas rep = rp::replicas(nrep, d.server_count);
        hipStream_t st = rp::as_stream(stream);
        rp::owner_load_walk(d.load_ws, n, nrep, d.id_bound, id_cap, d.M != 0, accumulate,
                            reinterpret_cast<unsigned long long*>(d_load), d.device, st,
                            [&](uint64_t k0, uint64_t cnt, uint32_t* rows) {
                                const rp::DevKeys c = rp::DevKeys{d_keys, d_off, stride, nullptr}.from(k0);
                                rp::launch_lookupn_view(d.view(), c.keys, c.off, c.stride, c.hashes, cnt, rep.np, rep.W,
                                                        rows, nullptr, st, rp::lookup_knobs().ablate);
                            });
    });
}

int rp_ring_owner_share(rp_ring* h, uint32_t id_cap, uint64_t* share) {
    return guard([&] {
        rp::Ring& r = R(h);
        svc_stop(r);
        rp::owner_share(r.view(), r.load_ws, r.nt.size(), id_cap, share, r.st);
    });
}

int rp_ring_snap_owner_share(rp_ring_snap* s, uint32_t id_cap, uint64_t* share) {
    return guard([&] {
        RP_REQUIRE(s, "null snapshot handle");
        rp::Snap& d = s->impl;
        RP_HIP(hipSetDevice(d.device));
        rp::owner_share(d.view(), d.load_ws, d.id_bound, id_cap, share, nullptr);
    });
}

// ---- moved ranges

int rp_ring_moved_ranges_dev(rp_ring* h, const rp_ring_snap* before, int32_t nrep, uint32_t cap, uint32_t* d_lo,
                             uint32_t* d_hi, uint32_t* d_before, uint32_t* d_after, uint32_t* d_count,
                             uint64_t* d_moved_hashes, void* stream) {
    return guard([&] {
        rp::Ring& r = R(h);
        const rp::Snap& s = S(before);
        RP_REQUIRE(s.device == r.device, "moved_ranges: the snapshot lives on another device");
        svc_stop(r);
        hipStream_t st = rp::as_stream(stream);
        // the ring is rebuilt on r.st; make the caller's stream wait for it
        if (st != r.st) RP_HIP(hipStreamSynchronize(r.st));
        rp::moved_ranges(s.view(), s.server_count, r.view(), r.server_count, r.range_ws, nrep, cap, d_lo, d_hi,
                         d_before, d_after, d_count, d_moved_hashes, st);
    });
}

int rp_ring_moved_ranges(rp_ring* h, const rp_ring_snap* before, int32_t nrep, uint32_t cap, uint32_t* lo,
                         uint32_t* hi, uint32_t* before_rows, uint32_t* after_rows, uint32_t* count,
                         uint64_t* moved_hashes) {
    return guard([&] {
        rp::Ring& r = R(h);
        const rp::Snap& s = S(before);
        RP_REQUIRE(s.device == r.device, "moved_ranges: the snapshot lives on another device");
        svc_stop(r);
        rp::host_moved_ranges(s.view(), s.server_count, r.view(), r.server_count, r.range_ws, nrep, cap, lo, hi,
                              before_rows, after_rows, count, moved_hashes, r.st);
    });
}

int rp_ring_snap_moved_ranges_dev(const rp_ring_snap* before, rp_ring_snap* after, int32_t nrep, uint32_t cap,
                                  uint32_t* d_lo, uint32_t* d_hi, uint32_t* d_before, uint32_t* d_after,
                                  uint32_t* d_count, uint64_t* d_moved_hashes, void* stream) {
    return guard([&] {
        const rp::Snap& b = S(before);
        RP_REQUIRE(after, "null snapshot handle");
        rp::Snap& a = after->impl;
        RP_REQUIRE(b.device == a.device, "moved_ranges: the snapshots live on different devices");
        RP_HIP(hipSetDevice(a.device));
        rp::moved_ranges(b.view(), b.server_count, a.view(), a.server_count, a.range_ws, nrep, cap, d_lo, d_hi,
                         d_before, d_after, d_count, d_moved_hashes, rp::as_stream(stream));
    });
}

int rp_ring_snap_moved_ranges(const rp_ring_snap* before, rp_ring_snap* after, int32_t nrep, uint32_t cap,
                              uint32_t* lo, uint32_t* hi, uint32_t* before_rows, uint32_t* after_rows,
                              uint32_t* count, uint64_t* moved_hashes) {
    return guard([&] {
        const rp::Snap& b = S(before);
        RP_REQUIRE(after, "null snapshot handle");
        rp::Snap& a = after->impl;
        RP_REQUIRE(b.device == a.device, "moved_ranges: the snapshots live on different devices");
        RP_HIP(hipSetDevice(a.device));
        rp::host_moved_ranges(b.view(), b.server_count, a.view(), a.server_count, a.range_ws, nrep, cap, lo, hi,
                              before_rows, after_rows, count, moved_hashes, nullptr);
    });
}

int rp_ring_snap_dump(const rp_ring_snap* s, uint32_t* tokens, uint32_t* owners, uint32_t cap) {
    return guard([&] {
        const rp::Snap& d = S(s);
        RP_HIP(hipSetDevice(d.device));
        const uint32_t n = std::min(cap, d.M);
        if (n) {
            if (tokens) RP_HIP(hipMemcpy(tokens, d.tok.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
            if (owners) RP_HIP(hipMemcpy(owners, d.own.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
        }
    });
}

// ---- farmhash + key generation

uint32_t rp_hash32(const char* s, size_t len) {
    return rp::fh::hash32(rp::fh::PtrSrc{reinterpret_cast<const uint8_t*>(s)}, (uint32_t)len);
}

int rp_hash32_batch_dev(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t* d_out, void* stream) {
    return guard([&] {
        if (!n) return;
        RP_REQUIRE(d_bytes && d_off && d_out, "hash32_batch_dev: null buffer");
        hipLaunchKernelGGL(rp::k_hash_batch, dim3(rp::grid_for(n, 256)), dim3(256), 0, rp::as_stream(stream), d_bytes,
                           d_off, n, d_out);
        RP_HIP(hipGetLastError());
    });
}

int rp_hash32_long_dev(const uint8_t* d_bytes, uint64_t len, uint32_t* d_out, void* stream) {
    return guard([&] {
        RP_REQUIRE(d_out && (d_bytes || len == 0), "hash32_long_dev: null buffer");
        RP_REQUIRE(len < (1ull << 32), "hash32_long_dev: at most 2^32-1 bytes");
        rp::hash_long(d_bytes, len, nullptr, nullptr, d_out, rp::as_stream(stream));
    });
}

int rp_hash32_long_multi_dev(const uint8_t* d_bytes, uint64_t stride, uint32_t n, uint32_t* d_meta, void* stream) {
    return guard([&] {
        RP_REQUIRE(n == 0 || (d_bytes && d_meta), "hash32_long_multi_dev: null buffer");
        rp::hash_long_multi(d_bytes, stride, n, d_meta, rp::as_stream(stream));
    });
}

int rp_gen_uuid_keys_dev(uint32_t seed, uint64_t k0, uint64_t n, uint8_t* d_out, void* stream) {
    return guard([&] {
        if (!n) return;
        RP_REQUIRE(d_out && (reinterpret_cast<uintptr_t>(d_out) & 3) == 0, "gen_uuid_keys_dev: need 4-byte aligned out");
        hipLaunchKernelGGL(rp::k_gen_uuid, dim3(rp::grid_for(n, 256, 8192)), dim3(256), 0, rp::as_stream(stream), seed,
                           k0, n, reinterpret_cast<uint32_t*>(d_out));
        RP_HIP(hipGetLastError());
    });
}

}  // extern "C"
