// Corpus retrieval for the two-tower rankers (include/neuroir_retrieve.h): the document index and the fused cosine top-k.
//
// Index layout (opaque to callers): documents in groups of 32, D padded to Dp = a multiple of 8.  Inside a group, for every block s of 8
// components and each half h of the block, the 32 documents' 4 components 8 s + 4 h .. + 3 lie side by side -- one wave reads block s of a group
// as 64 consecutive float4 and holds, per lane (document l & 31, half l >> 5), the A operands of the block's four v_mfma_f32_32x32x2_f32 steps.
// Step t of block s sums components 8 s + t and 8 s + 4 + t: the order of the D-sum is a fixed permutation of 0 .. Dp - 1, the same for every pair.
// Documents are the rows of a score tile and queries its columns, so a lane holds 16 scores of ONE query and compares them with that query's
// threshold in a register.
#include "common.hpp"
#include "../../include/neuroir_retrieve.h"
#include <math.h>
#include <algorithm>

namespace {
using namespace nir;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int RT_STEP = 128;          // documents per step of a workgroup: 4 waves x one 32-document group
constexpr int RT_CHUNK = 4096;        // documents per workgroup (nir_retrieve_chunk_docs)
constexpr int RT_TILE_LD = RT_STEP + 1, RT_MASK_LD = 5;      // LDS row strides (odd: the lanes of a wave are the queries)
constexpr int RT_SERIAL_K = 32;       // 64-query tiles fold lists up to this length by one lane per query; everything else by one wave per query
constexpr int MG_FAN = 31;            // lists merged per pass of the merge kernel: 31 inputs + the running result
constexpr size_t RT_LDS_MAX = 160 * 1024 - 1024;
enum { MODE_FUSED = 0, MODE_SCORES = 1, MODE_SELECT = 2 };

inline int pad_d(int D) { return (D + 7) & ~7; }

// float offset of component c of document d
__device__ __forceinline__ size_t elem_off(int64_t d, int c, int Dp) {
    return (size_t)(d >> 5) * (size_t)(32 * Dp) + (size_t)((c >> 3) * 256 + ((c >> 2) & 1) * 128 + (int)(d & 31) * 4 + (c & 3));
}

// the order of (value, index) pairs as one integer: the larger value first, the SMALLER index first among equal values; 0 = no entry
__device__ __forceinline__ u64 make_key(float v, int64_t idx) {
    uint32_t u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u64)u << 32) | (u64)(0xFFFFFFFFu - (uint32_t)idx);
}
__device__ __forceinline__ float key_val(u64 key) {
    if (key == 0ull) return -INFINITY;
    const uint32_t h = (uint32_t)(key >> 32);
    return __uint_as_float((h & 0x80000000u) ? (h ^ 0x80000000u) : ~h);
}
__device__ __forceinline__ int32_t key_idx(u64 key) { return key == 0ull ? -1 : (int32_t)(0xFFFFFFFFu - (uint32_t)key); }

// lanes of one wave hand values to each other through LDS: the hardware runs a wave's LDS operations in order, the compiler must too
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int CTRL>
__device__ __forceinline__ u64 dpp_mov64(u64 v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, true);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 readlane64(u64 v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 max64(u64 a, u64 b) { return a > b ? a : b; }
// all 64 lanes must be active (like wave_max of common.hpp, whose butterflies these are)
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
    v = max64(v, dpp_mov64<0xB1>(v));
    v = max64(v, dpp_mov64<0x4E>(v));
    v = max64(v, dpp_mov64<0x141>(v));
    v = max64(v, dpp_mov64<0x140>(v));
    return max64(max64(readlane64(v, 0), readlane64(v, 16)), max64(readlane64(v, 32), readlane64(v, 48)));
}

// One wave, one row y [D]: out[j] = component lane + 64 j of y / max(|y|, 1e-8) (0 beyond D); a row with a non-finite component gives zeros and
// returns true.  The sum of squares runs in an order that D alone fixes.  All 64 lanes must be active.
__device__ __forceinline__ bool unit_row(const float* y, int D, int lane, float out[4]) {
    float v[4];
    float n = 0.f;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane + 64 * j;
        v[j] = c < D ? y[c] : 0.f;
        bad |= (__float_as_uint(v[j]) & 0x7F800000u) == 0x7F800000u;
        n = fmaf(v[j], v[j], n);
    }
    n = fmaxf(sqrtf(wave_sum(n)), 1e-8f);
    bad = __ballot(bad) != 0ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = bad ? 0.f : v[j] / n;
    return bad;
}

__global__ __launch_bounds__(256) void retrieve_add_kernel(const float* reps, int64_t m, int D, int Dp, float* index, int64_t offset, int32_t* err) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;                 // wave-uniform
    float u[4];
    const bool bad = unit_row(reps + (size_t)row * D, D, lane, u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane + 64 * j;
        if (c < Dp) index[elem_off(offset + row, c, Dp)] = u[j];          // the padding components are zeros
    }
    if (bad && err && lane == 0) atomicOr(err, 1);
}

// plain [m, D] rows <-> the stored rows, bit for bit
template <bool IMPORT>
__global__ __launch_bounds__(256) void retrieve_rows_kernel(float* rows, int64_t m, int D, int Dp, float* index, int64_t offset) {
    const int64_t n = m * (int64_t)Dp;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / Dp;
        const int c = (int)(i - r * Dp);
        const size_t o = elem_off(offset + r, c, Dp);
        if (IMPORT)
            index[o] = c < D ? rows[(size_t)r * D + c] : 0.f;
        else if (c < D)
            rows[(size_t)r * D + c] = index[o];
    }
}

__global__ __launch_bounds__(256) void retrieve_fill_kernel(float* val, int32_t* idx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) val[i] = -INFINITY, idx[i] = -1;
}

// The 32 x 32 score tiles of one document group against NQ resident query tiles: acc[t][r] = score of query 32 t + (lane & 31) and document
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the group.  grp: the group's block of the index; qf: the query tiles in the same operand order (LDS).
// Document blocks are requested four ahead of the MFMAs that consume them.
template <int NQ>
__device__ __forceinline__ void score_tile(const float* grp, int nblk, const float* qf, int lane, f32x16 acc[NQ]) {
    const float4* dp = reinterpret_cast<const float4*>(grp) + lane;
    const float4* qp = reinterpret_cast<const float4*>(qf) + lane;
#pragma unroll
    for (int t = 0; t < NQ; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const auto block = [&](const float4& d, int sb) {
        if (sb >= nblk) return;           // wave-uniform
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            const float4 q = qp[(size_t)(t * nblk + sb) * 64];
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(d.x, q.x, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(d.y, q.y, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(d.z, q.z, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(d.w, q.w, acc[t], 0, 0, 0);
        }
    };
    // (a block beyond nblk is never consumed: its request is clamped into the group)
    float4 n0 = dp[0], n1 = dp[min(1, nblk - 1) * 64], n2 = dp[min(2, nblk - 1) * 64], n3 = dp[min(3, nblk - 1) * 64];
    for (int s = 0; s < nblk; s += 4) {
        const float4 c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        if (s + 4 < nblk) n0 = dp[(size_t)(s + 4) * 64];
        if (s + 5 < nblk) n1 = dp[(size_t)(s + 5) * 64];
        if (s + 6 < nblk) n2 = dp[(size_t)(s + 6) * 64];
        if (s + 7 < nblk) n3 = dp[(size_t)(s + 7) * 64];
        block(c0, s), block(c1, s + 1), block(c2, s + 2), block(c3, s + 3);
    }
}

struct TopkArgs {
    const float* queries;     // [B, D] raw
    const float* index;
    float* scores;            // plain form: [M, B] (document-major: a wave's 32 queries of one document are 128 consecutive bytes)
    int64_t B, M, chunks;
    int D, Dp, k;
    float* pval;              // [chunks, B, k]
    int32_t* pidx;
    int32_t* err;
};

// One wave folds the candidates that step `sb` left for query q (mask: which of the step's 128 documents passed the threshold; tile: their
// scores) into the query's sorted list: every old entry moves down by the number of candidates that beat it, every candidate lands at
// (old entries that beat it) + (candidates that beat it).  Keys are distinct, so the new positions are a permutation.
__device__ __forceinline__ void fold_candidates(int q, int64_t sb, int k, int lane, const float* tile, const uint32_t* mask, float* thr, int* cnt,
                                                volatile u64* L, volatile u64* ck) {
    const uint32_t m0 = mask[q * RT_MASK_LD + 0], m1 = mask[q * RT_MASK_LD + 1], m2 = mask[q * RT_MASK_LD + 2], m3 = mask[q * RT_MASK_LD + 3];
    const int p0 = __popc(m0), p1 = __popc(m1), p2 = __popc(m2), p3 = __popc(m3);
    const int c = p0 + p1 + p2 + p3;
    if (c == 0) return;                   // wave-uniform: every lane read the same words
    const int n = cnt[q];
    const u64 la = lane < n ? L[lane] : 0ull, lb = lane + 64 < n ? L[lane + 64] : 0ull;
    const int bit = lane & 31;
    const uint32_t below = (1u << bit) - 1u;
    const uint32_t wa = lane < 32 ? m0 : m1, wb = lane < 32 ? m2 : m3;
    const bool ha = (wa >> bit) & 1u, hb = (wb >> bit) & 1u;
    const u64 ka = ha ? make_key(tile[q * RT_TILE_LD + lane], sb + lane) : 0ull;
    const u64 kb = hb ? make_key(tile[q * RT_TILE_LD + 64 + lane], sb + 64 + lane) : 0ull;
    const int sa = (lane < 32 ? 0 : p0) + __popc(wa & below);
    const int sbb = p0 + p1 + (lane < 32 ? 0 : p2) + __popc(wb & below);
    if (ha) ck[sa] = ka;
    if (hb) ck[sbb] = kb;
    wave_sync();
    int ca = 0, cb = 0;
    for (int i = 0; i < c; ++i) {
        const u64 x = ck[i];
        const bool a_lt = la < x, b_lt = lb < x;
        ca += a_lt, cb += b_lt;
        const int below_x = __popcll(__ballot(lane < n && a_lt)) + __popcll(__ballot(lane + 64 < n && b_lt));
        const int rank = (n - below_x) + __popcll(__ballot(ka > x)) + __popcll(__ballot(kb > x));
        if (rank < k && lane == 0) L[rank] = x;
    }
    if (lane < n && lane + ca < k) L[lane + ca] = la;
    if (lane + 64 < n && lane + 64 + cb < k) L[lane + 64 + cb] = lb;
    const int n2 = min(k, n + c);
    wave_sync();
    if (lane == 0) {
        cnt[q] = n2;
        thr[q] = n2 == k ? key_val(L[k - 1]) : -INFINITY;
    }
    wave_sync();
}

// The same fold for a short list (k <= RT_SERIAL_K), one LANE per query: the candidates in document order, each inserted by shifting the
// smaller entries down.  64 queries fold side by side where the wave form above folds four; measured, that wins on a
// 64-query tile and loses on a 32-query one, where the wave form's four waves have 8 queries each.
__device__ __forceinline__ void fold_candidates_serial(int q, int64_t sb, int k, const float* tile, const uint32_t* mask, float* thr, int* cnt, u64* L) {
    int n = cnt[q];
    bool any = false;
    for (int w = 0; w < 4; ++w) {
        uint32_t word = mask[q * RT_MASK_LD + w];
        any |= word != 0u;
        while (word) {
            const int doc = 32 * w + __ffs((int)word) - 1;
            word &= word - 1u;
            const u64 key = make_key(tile[q * RT_TILE_LD + doc], sb + doc);
            if (n == k && !(key > L[k - 1])) continue;       // the threshold moved since the step began
            int pos = n < k ? n : k - 1;
            while (pos > 0 && L[pos - 1] < key) {
                L[pos] = L[pos - 1];
                --pos;
            }
            L[pos] = key;
            if (n < k) ++n;
        }
    }
    if (any) {
        cnt[q] = n;
        thr[q] = n == k ? key_val(L[k - 1]) : -INFINITY;
    }
}

// One workgroup per (chunk of RT_CHUNK documents, tile of 32 NQ queries).  MODE_FUSED: scores on the matrix pipe, selection behind a threshold
// compare, the chunk's k best per query out.  MODE_SCORES: the score tiles written to a.scores.  MODE_SELECT: the same selection, reading them back.
template <int NQ, int MODE>
__global__ __launch_bounds__(256) void retrieve_topk_kernel(TopkArgs a) {
    constexpr int QT = 32 * NQ;
    extern __shared__ __align__(16) char smem[];
    const int Dp = a.Dp, k = a.k, nblk = Dp >> 3;
    float* qf = reinterpret_cast<float*>(smem);                                    // [NQ][nblk][64] float4 (absent in MODE_SELECT)
    u64* lists = reinterpret_cast<u64*>(qf + (MODE == MODE_SELECT ? 0 : QT * Dp)); // [QT][k]
    u64* ck = lists + QT * k;                                                      // [4 waves][RT_STEP]
    float* tile = reinterpret_cast<float*>(ck + 4 * RT_STEP);                      // [QT][RT_TILE_LD]
    uint32_t* mask = reinterpret_cast<uint32_t*>(tile + QT * RT_TILE_LD);          // [QT][RT_MASK_LD]
    float* thr = reinterpret_cast<float*>(mask + QT * RT_MASK_LD);                 // [QT]
    int* cnt = reinterpret_cast<int*>(thr + QT);                                   // [QT]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t chunk = (int64_t)blockIdx.x % a.chunks;
    const int64_t q0 = ((int64_t)blockIdx.x / a.chunks) * QT;

    for (int q = threadIdx.x; q < QT; q += 256) thr[q] = -INFINITY, cnt[q] = 0;
    if (MODE != MODE_SELECT) {
        for (int q = w; q < QT; q += 4) {
            float u[4] = {0.f, 0.f, 0.f, 0.f};
            if (q0 + q < a.B && unit_row(a.queries + (size_t)(q0 + q) * a.D, a.D, lane, u) && a.err && chunk == 0 && lane == 0) atomicOr(a.err, 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = lane + 64 * j;
                if (c < Dp) qf[(q >> 5) * 32 * Dp + (c >> 3) * 256 + ((c >> 2) & 1) * 128 + (q & 31) * 4 + (c & 3)] = u[j];
            }
        }
    }
    __syncthreads();

    const int ql = lane & 31, half = lane >> 5;
    const int64_t end = min(a.M, (chunk + 1) * RT_CHUNK);
    for (int64_t sb = chunk * RT_CHUNK; sb < end; sb += RT_STEP) {
        const int64_t dbase = sb + 32 * w;             // this wave's document group
        f32x16 acc[NQ];
        if (dbase < a.M) {                             // wave-uniform; the group exists in the index: its capacity is a multiple of 32
            if (MODE == MODE_SELECT) {
#pragma unroll
                for (int t = 0; t < NQ; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t doc = dbase + (r & 3) + 8 * (r >> 2) + 4 * half, gq = q0 + 32 * t + ql;
                        acc[t][r] = (doc < a.M && gq < a.B) ? a.scores[(size_t)doc * a.B + gq] : 0.f;
                    }
            } else {
                score_tile<NQ>(a.index + (size_t)(dbase >> 5) * (size_t)(32 * Dp), nblk, qf, lane, acc);
            }
        }
        if (MODE == MODE_SCORES) {
            if (dbase < a.M) {
#pragma unroll
                for (int t = 0; t < NQ; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t doc = dbase + (r & 3) + 8 * (r >> 2) + 4 * half, gq = q0 + 32 * t + ql;
                        if (doc < a.M && gq < a.B) a.scores[(size_t)doc * a.B + gq] = acc[t][r];
                    }
            }
            continue;
        }
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            const int q = 32 * t + ql;
            uint32_t word = 0u;
            if (dbase < a.M && q0 + q < a.B) {
                const float th = thr[q];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int dl = (r & 3) + 8 * (r >> 2) + 4 * half;
                    const float s = acc[t][r] + 0.f;   // -0 -> +0: equal values have equal bits
                    // an equal score of a later document never displaces an entry: documents arrive in ascending order
                    if (dbase + dl < a.M && s > th) {
                        tile[q * RT_TILE_LD + 32 * w + dl] = s;
                        word |= 1u << dl;
                    }
                }
            }
            word |= (uint32_t)__shfl_xor((int)word, 32);
            if (half == 0) mask[q * RT_MASK_LD + w] = word;
        }
        __syncthreads();
        if (NQ == 2 && k <= RT_SERIAL_K) {
            if (threadIdx.x < QT) fold_candidates_serial(threadIdx.x, sb, k, tile, mask, thr, cnt, lists + threadIdx.x * k);
        } else {
            for (int q = w; q < QT; q += 4) fold_candidates(q, sb, k, lane, tile, mask, thr, cnt, lists + q * k, ck + w * RT_STEP);
        }
        __syncthreads();
    }
    if (MODE == MODE_SCORES) return;
    for (int q = w; q < QT; q += 4) {
        if (q0 + q >= a.B) continue;
        const int n = cnt[q];
        const size_t o = ((size_t)chunk * a.B + (size_t)(q0 + q)) * k;
        for (int i = lane; i < k; i += 64) {
            const u64 key = i < n ? lists[q * k + i] : 0ull;
            a.pval[o + i] = key_val(key);
            a.pidx[o + i] = key_idx(key);
        }
    }
}

// One wave per (query b, group g of F lists): the lists g F .. of vals / idx [P, B, k] merged into oval / oidx [groups, B, k].  Passes of
// MG_FAN lists: each of 31 lanes owns one list staged in LDS, lane 31 the result so far; k rounds of a wave-wide arg-max over the heads.
// The same (value, index) pair in two lists is emitted once.
__global__ __launch_bounds__(64) void retrieve_merge_kernel(const float* vals, const int32_t* idx, int P, int64_t B, int k, int F, float* oval,
                                                            int32_t* oidx) {
    __shared__ u64 slots[(MG_FAN + 1) * NIR_RETRIEVE_MAX_K];
    __shared__ u64 res[NIR_RETRIEVE_MAX_K];
    volatile u64* sl = slots;
    volatile u64* rs = res;
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int g = blockIdx.y;
    const int pend = min(P, (g + 1) * F);
    for (int i = lane; i < k; i += 64) sl[MG_FAN * k + i] = 0ull;
    for (int p0 = g * F; p0 < pend; p0 += MG_FAN) {
        const int nb = min(MG_FAN, pend - p0);
        for (int e = lane; e < nb * k; e += 64) {
            const int s = e / k, i = e - s * k;
            const size_t src = ((size_t)(p0 + s) * B + (size_t)b) * k + i;
            const int32_t ix = idx[src];
            sl[s * k + i] = ix < 0 ? 0ull : make_key(vals[src] + 0.f, ix);
        }
        wave_sync();
        const bool own = lane < nb || lane == MG_FAN;
        const int base = (lane < 32 ? lane : 0) * k;
        int cur = 0;
        u64 head = own ? sl[base] : 0ull;
        for (int r = 0; r < k; ++r) {
            const u64 best = wave_max_u64(head);
            if (lane == 0) rs[r] = best;
            if (best != 0ull && head == best) {
                ++cur;
                head = cur < k ? sl[base + cur] : 0ull;
            }
        }
        wave_sync();
        for (int i = lane; i < k; i += 64) sl[MG_FAN * k + i] = rs[i];
        wave_sync();
    }
    const size_t o = ((size_t)g * B + (size_t)b) * k;
    for (int i = lane; i < k; i += 64) {
        const u64 key = sl[MG_FAN * k + i];
        oval[o + i] = key_val(key);
        oidx[o + i] = key_idx(key);
    }
}

size_t topk_lds(int NQ, int mode, int Dp, int k) {
    const size_t QT = 32 * NQ;
    return (mode == MODE_SELECT ? 0 : QT * Dp * 4) + QT * k * 8 + 4 * RT_STEP * 8 + QT * RT_TILE_LD * 4 + QT * RT_MASK_LD * 4 + QT * 8;
}

// What a call does: the query tile width, the form, the lists per level of the merge and the workspace.
struct Plan {
    int NQ, plain;
    int64_t chunks, qtiles, groups;     // groups: lists after the first merge level (chunks > MG_FAN)
    size_t off_a, off_ai, off_b, off_bi, off_scores, bytes;
};

bool make_plan(int64_t B, int64_t M, int D, int k, int form, Plan& p) {
    if (B < 0 || B >= (1ll << 31) || M < 0 || M >= (1ll << 31) || D < 1 || D > NIR_RETRIEVE_MAX_D || k < 1 || k > NIR_RETRIEVE_MAX_K) return false;
    if (form != NIR_RETRIEVE_AUTO && form != NIR_RETRIEVE_FUSED && form != NIR_RETRIEVE_PLAIN) return false;
    const int Dp = pad_d(D);
    p.plain = form == NIR_RETRIEVE_PLAIN;
    p.NQ = (B > 32 && topk_lds(2, MODE_FUSED, Dp, k) <= RT_LDS_MAX) ? 2 : 1;
    p.chunks = (M + RT_CHUNK - 1) / RT_CHUNK;
    p.qtiles = (B + 32 * p.NQ - 1) / (32 * p.NQ);
    if (p.chunks * p.qtiles >= (1ll << 31)) return false;
    p.groups = (p.chunks + MG_FAN - 1) / MG_FAN;
    Workspace ws(nullptr, 0);
    const size_t na = p.chunks > 1 ? (size_t)p.chunks * B * k : 0, nb = p.chunks > MG_FAN ? (size_t)p.groups * B * k : 0;
    ws.take<float>(na), p.off_a = ws.off - na * 4;
    ws.take<int32_t>(na), p.off_ai = ws.off - na * 4;
    ws.take<float>(nb), p.off_b = ws.off - nb * 4;
    ws.take<int32_t>(nb), p.off_bi = ws.off - nb * 4;
    const size_t ns = p.plain ? (size_t)M * B : 0;
    ws.take<float>(ns), p.off_scores = ws.off - ns * 4;
    p.bytes = align_up(ws.off, 256);
    return true;
}

template <int NQ, int MODE>
int launch_topk(const TopkArgs& a, int64_t blocks, hipStream_t st, const char* name) {
    const size_t lds = topk_lds(NQ, MODE, a.Dp, a.k);
    if (lds > 64 * 1024) {     // once per device and kernel (an index lives on any device): the largest size the entry uses
        static std::atomic<unsigned long long> done{0ull};
        int dev = 0;
        hipGetDevice(&dev);
        const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
        if (!(done.load(std::memory_order_acquire) & bit) || bit == 0ull) {
            const hipError_t e =
                hipFuncSetAttribute((const void*)retrieve_topk_kernel<NQ, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RT_LDS_MAX);
            if (e != hipSuccess) {
                set_error("retrieve_topk: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e));
                return (int)e;
            }
            done.fetch_or(bit, std::memory_order_release);
        }
    }
    ProfScope ps(name, st);
    hipLaunchKernelGGL((retrieve_topk_kernel<NQ, MODE>), dim3((unsigned)blocks), dim3(256), lds, st, a);
    NIR_CHECK_LAUNCH(name);
    return 0;
}

int launch_merge(const float* vals, const int32_t* idx, int64_t P, int64_t B, int k, int F, int64_t groups, float* oval, int32_t* oidx, hipStream_t st) {
    ProfScope ps("retrieve_merge_kernel", st);
    hipLaunchKernelGGL(retrieve_merge_kernel, dim3((unsigned)B, (unsigned)groups), dim3(64), 0, st, vals, idx, (int)P, B, k, F, oval, oidx);
    NIR_CHECK_LAUNCH("nir_retrieve_merge");
    return 0;
}

bool index_args_ok(int64_t capacity, int D, int64_t offset, int64_t m) {
    return capacity >= 0 && capacity < (1ll << 31) && D >= 1 && D <= NIR_RETRIEVE_MAX_D && offset >= 0 && m >= 0 && offset <= capacity &&
           m <= capacity - offset;
}
}  // namespace

extern "C" int nir_retrieve_chunk_docs(void) { return RT_CHUNK; }

extern "C" size_t nir_retrieve_index_bytes(int64_t capacity, int D) {
    if (!index_args_ok(capacity, D, 0, 0)) return 0;
    return align_up((size_t)((capacity + 31) / 32) * 32 * (size_t)pad_d(D) * 4, 256);
}

extern "C" int nir_retrieve_add(const float* reps, int64_t m, int D, void* index, int64_t capacity, int64_t offset, int32_t* err_flag,
                                nir_stream_t stream) {
    NIR_REQUIRE(index_args_ok(capacity, D, offset, m), "retrieve_add: D %d outside 1 .. %d, or documents %lld .. +%lld outside the capacity %lld", D,
                NIR_RETRIEVE_MAX_D, (long long)offset, (long long)m, (long long)capacity);
    if (m == 0) return 0;
    NIR_REQUIRE(reps && index, "retrieve_add: null pointer");
    NIR_REQUIRE(((uintptr_t)index & 15) == 0, "retrieve_add: the index must be 16-byte aligned");
    ProfScope ps("retrieve_add_kernel", (hipStream_t)stream);
    hipLaunchKernelGGL(retrieve_add_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream, reps, m, D, pad_d(D), (float*)index, offset,
                       err_flag);
    NIR_CHECK_LAUNCH("nir_retrieve_add");
    return 0;
}

extern "C" int nir_retrieve_export(const void* index, int64_t capacity, int D, int64_t offset, int64_t m, float* rows, nir_stream_t stream) {
    NIR_REQUIRE(index_args_ok(capacity, D, offset, m), "retrieve_export: D %d outside 1 .. %d, or documents %lld .. +%lld outside the capacity %lld", D,
                NIR_RETRIEVE_MAX_D, (long long)offset, (long long)m, (long long)capacity);
    if (m == 0) return 0;
    NIR_REQUIRE(rows && index, "retrieve_export: null pointer");
    const int Dp = pad_d(D);
    const int64_t blocks = std::min<int64_t>((m * Dp + 255) / 256, 1 << 20);
    ProfScope ps("retrieve_rows_kernel", (hipStream_t)stream);
    hipLaunchKernelGGL(retrieve_rows_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, m, D, Dp, (float*)index, offset);
    NIR_CHECK_LAUNCH("nir_retrieve_export");
    return 0;
}

extern "C" int nir_retrieve_import(const float* rows, int64_t m, int D, void* index, int64_t capacity, int64_t offset, nir_stream_t stream) {
    NIR_REQUIRE(index_args_ok(capacity, D, offset, m), "retrieve_import: D %d outside 1 .. %d, or documents %lld .. +%lld outside the capacity %lld", D,
                NIR_RETRIEVE_MAX_D, (long long)offset, (long long)m, (long long)capacity);
    if (m == 0) return 0;
    NIR_REQUIRE(rows && index, "retrieve_import: null pointer");
    const int Dp = pad_d(D);
    const int64_t blocks = std::min<int64_t>((m * Dp + 255) / 256, 1 << 20);
    ProfScope ps("retrieve_rows_kernel", (hipStream_t)stream);
    hipLaunchKernelGGL(retrieve_rows_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float*)rows, m, D, Dp, (float*)index, offset);
    NIR_CHECK_LAUNCH("nir_retrieve_import");
    return 0;
}

extern "C" size_t nir_retrieve_topk_workspace_bytes(int64_t B, int64_t M, int D, int k, int form) {
    Plan p;
    return make_plan(B, M, D, k, form, p) ? p.bytes : 0;
}

extern "C" int nir_retrieve_topk(const float* queries, int64_t B, const void* index, int64_t M, int D, int k, int form, void* workspace,
                                 size_t workspace_bytes, int32_t* err_flag, float* top_val, int32_t* top_idx, nir_stream_t stream) {
    Plan p;
    NIR_REQUIRE(make_plan(B, M, D, k, form, p),
                "retrieve_topk: B %lld / M %lld outside [0, 2^31) (or B x M beyond one launch), D %d outside 1 .. %d, k %d outside 1 .. %d, or form %d unknown",
                (long long)B, (long long)M, D, NIR_RETRIEVE_MAX_D, k, NIR_RETRIEVE_MAX_K, form);
    if (B == 0) return 0;
    NIR_REQUIRE(queries && top_val && top_idx && (index || M == 0), "retrieve_topk: null pointer");
    NIR_REQUIRE(((uintptr_t)index & 15) == 0, "retrieve_topk: the index must be 16-byte aligned");
    if (p.bytes > 0 && (!workspace || workspace_bytes < p.bytes)) {
        set_error("retrieve_topk: workspace too small (%zu < %zu bytes)", workspace ? workspace_bytes : (size_t)0, p.bytes);
        return NIR_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (M == 0) {
        ProfScope ps("retrieve_fill_kernel", st);
        hipLaunchKernelGGL(retrieve_fill_kernel, g1(B * k), dim3(256), 0, st, top_val, top_idx, B * k);
        NIR_CHECK_LAUNCH("nir_retrieve_topk (fill)");
        return 0;
    }
    char* ws = (char*)workspace;
    float* la = p.chunks > 1 ? (float*)(ws + p.off_a) : top_val;
    int32_t* lai = p.chunks > 1 ? (int32_t*)(ws + p.off_ai) : top_idx;
    TopkArgs a{queries, (const float*)index, p.plain ? (float*)(ws + p.off_scores) : nullptr, B, M, p.chunks, D, pad_d(D), k, la, lai, err_flag};
    const int64_t blocks = p.chunks * p.qtiles;
    if (p.plain) {
        NIR_PROPAGATE((p.NQ == 2 ? launch_topk<2, MODE_SCORES>(a, blocks, st, "retrieve_scores_kernel")
                                 : launch_topk<1, MODE_SCORES>(a, blocks, st, "retrieve_scores_kernel")));
        NIR_PROPAGATE((p.NQ == 2 ? launch_topk<2, MODE_SELECT>(a, blocks, st, "retrieve_select_kernel")
                                 : launch_topk<1, MODE_SELECT>(a, blocks, st, "retrieve_select_kernel")));
    } else {
        NIR_PROPAGATE((p.NQ == 2 ? launch_topk<2, MODE_FUSED>(a, blocks, st, "retrieve_topk_kernel")
                                 : launch_topk<1, MODE_FUSED>(a, blocks, st, "retrieve_topk_kernel")));
    }
    // the chunks' lists -> one list per query, MG_FAN lists per wave and level; the levels alternate between the two list buffers
    const float* src = la;
    const int32_t* srci = lai;
    int64_t P = p.chunks;
    bool to_b = true;
    while (P > 1) {
        const int64_t G = (P + MG_FAN - 1) / MG_FAN;
        float* dst = G == 1 ? top_val : (float*)(ws + (to_b ? p.off_b : p.off_a));
        int32_t* dsti = G == 1 ? top_idx : (int32_t*)(ws + (to_b ? p.off_bi : p.off_ai));
        NIR_PROPAGATE(launch_merge(src, srci, P, B, k, MG_FAN, G, dst, dsti, st));
        src = dst, srci = dsti, P = G, to_b = !to_b;
    }
    return 0;
}

extern "C" int nir_retrieve_merge(const float* vals, const int32_t* idx, int P, int64_t B, int k, float* out_val, int32_t* out_idx,
                                  nir_stream_t stream) {
    NIR_REQUIRE(P >= 1 && P < (1 << 20) && B >= 0 && B < (1ll << 31) && k >= 1 && k <= NIR_RETRIEVE_MAX_K,
                "retrieve_merge: P %d outside [1, 2^20), B %lld outside [0, 2^31) or k %d outside 1 .. %d", P, (long long)B, k, NIR_RETRIEVE_MAX_K);
    if (B == 0) return 0;
    NIR_REQUIRE(vals && idx && out_val && out_idx, "retrieve_merge: null pointer");
    return launch_merge(vals, idx, P, B, k, P, 1, out_val, out_idx, (hipStream_t)stream);
}
