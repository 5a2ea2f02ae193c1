// Grouped teacher-forced attention (include/neuroir_teacher.h): Luong general / dot attention for the decoder rows of ALL
// teacher-forced steps of all candidates at once.  The G = N (TL - 1) rows of a decode row share one memory bank, one score bank and one length:
//   S = h sb^T -> mask -> softmax -> ctx = P mem;  cat = [ctx ; h];  the attention row P (optional)
//   fused: one workgroup per (group, block of 64 rows), both banks as fp16 term planes in LDS, both products on the matrix cores   tf_attend_fused_kernel
//   plain: one wave per row, fp32 VALU -- s2s_attend_kernel's body (csrc/seq2seq.hip) with the group mapping                        tf_attend_plain_kernel
// Everything is enqueued on the caller's stream: no host synchronisation, no allocation, no atomics, every reduction in a fixed order.
#include <algorithm>
#include "split2.hpp"

namespace nir {

#ifndef NIR_TF_WAVES
#define NIR_TF_WAVES 4                            // measured against 2 and 8: tools build those as NIR_VARIANT libraries
#endif
constexpr int TF_WAVES = NIR_TF_WAVES, TF_THREADS = 64 * TF_WAVES;
constexpr int TF_ROWS = 16 * TF_WAVES;            // rows of a workgroup: four waves, one 16-row MFMA tile each
constexpr int TF_MAX_QL = 64;                     // the fused form keeps a row's scores in registers: at most four 16-position tiles
constexpr size_t TF_LDS_BYTES = (size_t)160 << 10;
// rows per group from which the entry takes the fused form (measured): both forms move the same bytes -- h in, cat out --
// and the plain form's bank reads hit L2; staging a bank pays once a group fills two row blocks (plain ahead up to 108 rows, fused at 180)
constexpr int64_t TF_MIN_G = 128;

static inline int tf_up(int x, int m) { return (x + m - 1) / m * m; }
// LDS image of the fused form, in fp16 elements: [2 terms][QLp][H + 8] score bank (position-major: the A operand of S), [2][H][QLp] memory bank
// (feature-major: the A operand of ctx, its QL axis zero-filled up to QLp), [TF_WAVES][2][16][QLk + 8] probabilities.  QLp = ceil16(QL), QLk =
// ceil32(QL).  The memory bank's rows carry no pad: at the headline shape (H 512, QL 10) the image is 71 KB, two workgroups a CU, where eight
// more columns made it 87 KB and one (its reads are two-way conflicted at QLp 16; the second workgroup is worth more).
static inline int tf_ldj(int QL, int H) { (void)H; return tf_up(QL, 16); }
static inline size_t tf_lds_bytes(int QL, int H) {
    const size_t QLp = tf_up(QL, 16), QLk = tf_up(QL, 32);
    return (2 * QLp * (H + 8) + 2 * (size_t)H * tf_ldj(QL, H) + TF_WAVES * 2 * 16 * (QLk + 8)) * sizeof(_Float16);
}
static inline bool tf_fusable(int QL, int H) {
    return H % 32 == 0 && H >= 32 && H <= 1024 && QL >= 1 && QL <= TF_MAX_QL && tf_lds_bytes(QL, H) <= TF_LDS_BYTES;
}

__device__ __forceinline__ f16x8 tf_pack(const uint2 a, const uint2 b) { return __builtin_bit_cast(f16x8, make_uint4(a.x, a.y, b.x, b.y)); }

// ---- fused form ---------------------------------------------------------------------------------------------------------------------------------
// blockIdx.x = g nblk + blk; wave w owns rows blk 64 + 16 w .. + 15 of group g, lane (c16, g4) row c16 of them.  Both products put the bank on
// the A side, so a lane's accumulator registers belong to ONE row: S gives it the scores of positions jt 16 + 4 g4 + r (the softmax combines
// the four lanes of a row with two xor steps), ctx the features nt 16 + 4 g4 + r (one float4 store).  h never touches LDS: a lane loads the
// eight values of its B fragment from global, splits them in registers and writes them to cat's second half on the way.  Rows past G load row
// G - 1 and store nothing; a wave without rows leaves behind the staging barrier.
template <int NJT>
__global__ __launch_bounds__(TF_THREADS, 1) void tf_attend_fused_kernel(const float* __restrict__ h, const float* __restrict__ mem, const float* __restrict__ sb,
                                                                 const int64_t* __restrict__ lens, const int64_t* __restrict__ rowmap, int64_t G, int nblk,
                                                                 int64_t rows_src, int QL, int H, int LDJ, float* __restrict__ cat,
                                                                 float* __restrict__ attn, int64_t attn_stride) {
    extern __shared__ __attribute__((aligned(16))) _Float16 tf_sm[];
    constexpr int QLp = 16 * NJT, KT2 = (NJT + 1) / 2, QLk = 32 * KT2, LDP = QLk + 8;
    const int LDH = H + 8, KS = H / 32, H4 = H / 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g4 = lane >> 4;
    const int64_t g = blockIdx.x / nblk;
    const int blk = (int)(blockIdx.x - g * nblk);
    int64_t src = rowmap ? rowmap[g] : g;
    src = src < 0 ? 0 : (src >= rows_src ? rows_src - 1 : src);
    const int64_t ln = lens[src];
    const int len = ln < 0 ? 0 : (ln > QL ? QL : (int)ln);
    _Float16* sbp = tf_sm;                                       // [2][QLp][LDH]
    _Float16* mtp = sbp + 2 * QLp * LDH;                         // [2][H][LDJ]
    _Float16* pw = mtp + 2 * H * LDJ + wave * 2 * 16 * LDP;      // [2][16][LDP] of this wave
    {
        const float* sg = sb + src * QL * H;
        const float* mg = mem + src * QL * H;
        constexpr int SB = 4;                                                     // float4 pairs in flight before the first is written
        const int total = QLp * H4;
        for (int e0 = tid; e0 < total; e0 += TF_THREADS * SB) {
            float4 av[SB], bv[SB];
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                const int e = min(e0 + TF_THREADS * q, total - 1);
                const int j = min(e / H4, QL - 1), c = e % H4;                   // clamped: a padded position is zeroed below
                av[q] = *reinterpret_cast<const float4*>(sg + (int64_t)j * H + 4 * c);
                bv[q] = *reinterpret_cast<const float4*>(mg + (int64_t)j * H + 4 * c);
            }
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                const int e = e0 + TF_THREADS * q;
                if (e < total) {
                    const int j = e / H4, c = e - j * H4;
                    float4 a = av[q], b = bv[q];
                    if (j >= QL) a = b = make_float4(0.f, 0.f, 0.f, 0.f);
                    const Split2x4 sa = split2(a);
                    *reinterpret_cast<uint2*>(sbp + j * LDH + 4 * c) = sa.hi;
                    *reinterpret_cast<uint2*>(sbp + (QLp + j) * LDH + 4 * c) = sa.lo;
                    const Split2x2 b01 = split2(b.x, b.y), b23 = split2(b.z, b.w);
                    _Float16* m0 = mtp + (4 * c) * LDJ + j;
                    _Float16* m1 = m0 + H * LDJ;
                    m0[0] = (_Float16)b01.hi[0]; m0[LDJ] = (_Float16)b01.hi[1]; m0[2 * LDJ] = (_Float16)b23.hi[0]; m0[3 * LDJ] = (_Float16)b23.hi[1];
                    m1[0] = (_Float16)b01.lo[0]; m1[LDJ] = (_Float16)b01.lo[1]; m1[2 * LDJ] = (_Float16)b23.lo[0]; m1[3 * LDJ] = (_Float16)b23.lo[1];
                }
            }
        }
    }
    __syncthreads();
    const int64_t row0 = (int64_t)blk * TF_ROWS + wave * 16;
    if (row0 >= G) return;                                                    // wave-uniform; no barrier below
    const int64_t row = row0 + c16;
    const bool row_ok = row < G;
    const int64_t gr = g * G + (row_ok ? row : G - 1);                        // the row this lane loads
    const float* hr = h + gr * H + 8 * g4;
    float* cr = cat + gr * 2 * H;
    // ---- S = sb h^T: scores of positions jt 16 + 4 g4 + r of row c16 ----
    f32x4 acc[NJT], acx[NJT];
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) { acc[jt] = (f32x4){0.f, 0.f, 0.f, 0.f}; acx[jt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    const _Float16* sp0 = sbp + c16 * LDH + 8 * g4;
    // h in chunks of TF_KC k-steps, the next chunk's loads in flight under this chunk's products (one wave per SIMD hides nothing else)
    constexpr int TF_KC = 4;
    const int NCH = (KS + TF_KC - 1) / TF_KC;
    auto load_h = [&](int c, float4 (&hb)[TF_KC][2]) {
#pragma unroll
        for (int u = 0; u < TF_KC; ++u) {
            const int ks = min(c * TF_KC + u, KS - 1);                            // clamped: a duplicate k-step is not multiplied below
            hb[u][0] = *reinterpret_cast<const float4*>(hr + 32 * ks);
            hb[u][1] = *reinterpret_cast<const float4*>(hr + 32 * ks + 4);
        }
    };
    auto products = [&](int c, const float4 (&hb)[TF_KC][2]) {
#pragma unroll
        for (int u = 0; u < TF_KC; ++u) {
            const int ks = c * TF_KC + u;
            if (ks < KS) {                                                        // wave-uniform
                const Split2x4 s0 = split2(hb[u][0]), s1 = split2(hb[u][1]);
                const f16x8 bh = tf_pack(s0.hi, s1.hi), bl = tf_pack(s0.lo, s1.lo);
                if (row_ok) {
                    *reinterpret_cast<float4*>(cr + H + 32 * ks + 8 * g4) = hb[u][0];
                    *reinterpret_cast<float4*>(cr + H + 32 * ks + 8 * g4 + 4) = hb[u][1];
                }
#pragma unroll
                for (int jt = 0; jt < NJT; ++jt) {
                    const f16x8 w0 = *reinterpret_cast<const f16x8*>(sp0 + jt * 16 * LDH + 32 * ks);
                    const f16x8 w1 = *reinterpret_cast<const f16x8*>(sp0 + (QLp + jt * 16) * LDH + 32 * ks);
                    acx[jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, bh, acx[jt], 0, 0, 0);
                    acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, bh, acc[jt], 0, 0, 0);
                    acx[jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, bl, acx[jt], 0, 0, 0);
                }
            }
        }
    };
    {
        float4 hA[TF_KC][2], hB[TF_KC][2];
        load_h(0, hA);
        for (int c = 0; c < NCH; c += 2) {
            if (c + 1 < NCH) load_h(c + 1, hB);
            products(c, hA);
            if (c + 1 >= NCH) break;
            if (c + 2 < NCH) load_h(c + 2, hA);
            products(c + 1, hB);
        }
    }
    // ---- mask, softmax (fp32, registers): lanes l, l + 16, l + 32, l + 48 hold the same row ----
    float p[NJT][4];
    float mx = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[jt][r] = split2_combine(acc[jt][r], acx[jt][r]);
            if (jt * 16 + 4 * g4 + r < len) mx = fmaxf(mx, p[jt][r]);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float den = 0.f;
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[jt][r] = jt * 16 + 4 * g4 + r < len ? expf(p[jt][r] - mx) : 0.f;
            den += p[jt][r];
        }
    }
    den += __shfl_xor(den, 16);
    den += __shfl_xor(den, 32);
    const float inv = 1.f / den;                                              // len >= 1: den >= 1 (the largest score's term is exp(0))
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) p[jt][r] = p[jt][r] * inv;
    }
    if (attn && row_ok) {
        float* ar = attn + gr * attn_stride;
#pragma unroll
        for (int jt = 0; jt < NJT; ++jt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = jt * 16 + 4 * g4 + r;
                if (j < QL) ar[j] = len == 0 ? NAN : p[jt][r];
            }
        }
    }
    // ---- P as fp16 term pairs through this wave's LDS tile (a transposition: the B fragment wants eight positions of one row) ----
#pragma unroll
    for (int jt = 0; jt < 2 * KT2; ++jt) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (jt < NJT && len > 0) v = make_float4(p[jt < NJT ? jt : 0][0], p[jt < NJT ? jt : 0][1], p[jt < NJT ? jt : 0][2], p[jt < NJT ? jt : 0][3]);
        const Split2x4 sv = split2(v);
        *reinterpret_cast<uint2*>(pw + c16 * LDP + jt * 16 + 4 * g4) = sv.hi;
        *reinterpret_cast<uint2*>(pw + (16 + c16) * LDP + jt * 16 + 4 * g4) = sv.lo;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    f16x8 pb[KT2][2];
#pragma unroll
    for (int kt = 0; kt < KT2; ++kt) {
        pb[kt][0] = *reinterpret_cast<const f16x8*>(pw + c16 * LDP + 32 * kt + 8 * g4);
        pb[kt][1] = *reinterpret_cast<const f16x8*>(pw + (16 + c16) * LDP + 32 * kt + 8 * g4);
    }
    // ---- ctx = mem^T P^T: features nt 16 + 4 g4 + r of row c16 ----
    const f16x8 zero8 = __builtin_bit_cast(f16x8, make_uint4(0u, 0u, 0u, 0u));
    const _Float16* mp0 = mtp + c16 * LDJ + 8 * g4;
    for (int nt = 0; nt < H / 16; ++nt) {
        f32x4 cc = (f32x4){0.f, 0.f, 0.f, 0.f}, cx = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < KT2; ++kt) {
            f16x8 m0 = zero8, m1 = zero8;
            if (32 * kt + 8 * g4 < QLp) {                                     // positions past QLp are not in the image: zeros from registers
                m0 = *reinterpret_cast<const f16x8*>(mp0 + nt * 16 * LDJ + 32 * kt);
                m1 = *reinterpret_cast<const f16x8*>(mp0 + (H + nt * 16) * LDJ + 32 * kt);
            }
            cx = __builtin_amdgcn_mfma_f32_16x16x32_f16(m1, pb[kt][0], cx, 0, 0, 0);
            cc = __builtin_amdgcn_mfma_f32_16x16x32_f16(m0, pb[kt][0], cc, 0, 0, 0);
            cx = __builtin_amdgcn_mfma_f32_16x16x32_f16(m0, pb[kt][1], cx, 0, 0, 0);
        }
        if (row_ok) {
            f32x4 o = split2_combine(cc, cx);
            if (len == 0) o = (f32x4){NAN, NAN, NAN, NAN};
            *reinterpret_cast<f32x4*>(cr + nt * 16 + 4 * g4) = o;
        }
    }
}

// ---- plain form: one wave per row (s2s_attend_kernel's general / dot body, restated with the group mapping) -----------------------------------------
__global__ __launch_bounds__(256) void tf_attend_plain_kernel(const float* __restrict__ h, const float* __restrict__ mem, const float* __restrict__ sb,
                                                              const int64_t* __restrict__ lens, const int64_t* __restrict__ rowmap, int64_t R, int64_t G,
                                                              int64_t rows_src, int QL, int H, float* __restrict__ cat, float* __restrict__ attn,
                                                              int64_t attn_stride) {
    extern __shared__ float tf_pr[];                  // [4][QL]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= R) return;
    float* pw = tf_pr + wave * QL;
    const int64_t g = i / G;
    int64_t si = rowmap ? rowmap[g] : g;
    si = si < 0 ? 0 : (si >= rows_src ? rows_src - 1 : si);
    const int64_t ln = lens[si];
    const int len = ln < 0 ? 0 : (ln > QL ? QL : (int)ln);
    const float* mb = mem + si * QL * H;
    const float* sq = sb + si * QL * H;
    const float* qi = h + i * H;
    float mx = -INFINITY;
    for (int j = 0; j < len; ++j) {
        float s = 0.f;
        for (int f = 4 * lane; f < H; f += 256) {
            const float4 a = *reinterpret_cast<const float4*>(sq + (int64_t)j * H + f), b = *reinterpret_cast<const float4*>(qi + f);
            s += (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
        }
        s = wave_sum(s);
        if (lane == 0) pw[j] = s;
        mx = fmaxf(mx, s);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float den = 0.f;
    for (int j = 0; j < len; ++j) den += expf(pw[j] - mx);
    if (attn) {
        float* ar = attn + i * attn_stride;
        for (int j = lane; j < QL; j += 64) ar[j] = len == 0 ? NAN : (j < len ? expf(pw[j] - mx) / den : 0.0f);
    }
    float* o = cat + i * 2 * H;
    for (int f = 4 * lane; f < H; f += 256) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < len; ++j) {
            const float p = expf(pw[j] - mx) / den;
            const float4 x = *reinterpret_cast<const float4*>(mb + (int64_t)j * H + f);
            acc.x = fmaf(p, x.x, acc.x); acc.y = fmaf(p, x.y, acc.y); acc.z = fmaf(p, x.z, acc.z); acc.w = fmaf(p, x.w, acc.w);
        }
        if (len == 0) acc = make_float4(NAN, NAN, NAN, NAN);
        *reinterpret_cast<float4*>(o + f) = acc;
        *reinterpret_cast<float4*>(o + H + f) = *reinterpret_cast<const float4*>(qi + f);
    }
}

template <int NJT>
static int launch_tf_fused(const float* h, const float* mem, const float* sb, const int64_t* lens, const int64_t* rowmap, int64_t ngroups, int64_t G,
                           int64_t rows_src, int QL, int H, float* cat, float* attn, int64_t attn_stride, hipStream_t st) {
    static const hipError_t raised =
        hipFuncSetAttribute((const void*)tf_attend_fused_kernel<NJT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TF_LDS_BYTES);
    (void)raised;
    const int64_t nblk = (G + TF_ROWS - 1) / TF_ROWS;
    {
        ProfScope ps(prof_shape_name("tf_attend_fused_kernel", (long long)(ngroups * G), QL, H), st);
        hipLaunchKernelGGL(tf_attend_fused_kernel<NJT>, dim3((unsigned)(ngroups * nblk)), dim3(TF_THREADS), tf_lds_bytes(QL, H), st, h, mem, sb, lens, rowmap, G,
                           (int)nblk, rows_src, QL, H, tf_ldj(QL, H), cat, attn, attn_stride);
    }
    NIR_CHECK_LAUNCH("tf_attend_fused_kernel");
    return 0;
}

}  // namespace nir

extern "C" int nir_tf_attend_fusable(int QL, int H, int same_bank) {
    (void)same_bank;                                  // the dot form stages its one bank in both layouts: the same image, the same rule
    return nir::tf_fusable(QL, H) ? 1 : 0;
}

extern "C" size_t nir_tf_attend_workspace_bytes(int64_t ngroups, int64_t G, int QL, int H) {
    (void)ngroups; (void)G; (void)QL; (void)H;
    return 0;
}

extern "C" int nir_tf_attend(const float* h, const float* memory_bank, const float* score_bank, const int64_t* source_len, const int64_t* rowmap,
                             int64_t ngroups, int64_t G, int64_t rows_src, int QL, int H, float* cat, float* attn, int64_t attn_stride, void* workspace,
                             size_t workspace_bytes, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(h && memory_bank && score_bank && source_len && cat, "tf_attend: null pointer");
    NIR_REQUIRE(ngroups >= 0 && G >= 0 && (G == 0 || ngroups < 0x7FFFFFFFLL / G), "tf_attend: ngroups / G negative or ngroups G >= 2^31");
    NIR_REQUIRE(H >= 4 && H <= 8192 && H % 4 == 0, "tf_attend: H outside [4, 8192] or no multiple of 4");
    NIR_REQUIRE(QL >= 1 && QL <= 4096, "tf_attend: QL outside [1, 4096]");
    NIR_REQUIRE(!attn || attn_stride >= QL, "tf_attend: attn_stride below QL");
    if (ngroups == 0 || G == 0) return 0;
    NIR_REQUIRE(rows_src > 0, "tf_attend: rows_src <= 0 with rows to do");
    NIR_REQUIRE(rowmap || ngroups <= rows_src, "tf_attend: more groups than bank rows without a rowmap");
    const size_t need = nir_tf_attend_workspace_bytes(ngroups, G, QL, H);
    if (need && (!workspace || workspace_bytes < need)) {
        set_error("tf_attend: workspace null or too small");
        return NIR_ERR_WORKSPACE;
    }
    if (tf_fusable(QL, H) && G >= TF_MIN_G && !tun(g_tun.exact_f32)) {
        switch ((QL + 15) / 16) {
            case 1: return launch_tf_fused<1>(h, memory_bank, score_bank, source_len, rowmap, ngroups, G, rows_src, QL, H, cat, attn, attn_stride, st);
            case 2: return launch_tf_fused<2>(h, memory_bank, score_bank, source_len, rowmap, ngroups, G, rows_src, QL, H, cat, attn, attn_stride, st);
            case 3: return launch_tf_fused<3>(h, memory_bank, score_bank, source_len, rowmap, ngroups, G, rows_src, QL, H, cat, attn, attn_stride, st);
            default: return launch_tf_fused<4>(h, memory_bank, score_bank, source_len, rowmap, ngroups, G, rows_src, QL, H, cat, attn, attn_stride, st);
        }
    }
    const int64_t R = ngroups * G;
    {
        ProfScope ps("tf_attend_plain_kernel", st);
        hipLaunchKernelGGL(tf_attend_plain_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), (size_t)4 * QL * sizeof(float), st, h, memory_bank, score_bank,
                           source_len, rowmap, R, G, rows_src, QL, H, cat, attn, attn_stride);
    }
    NIR_CHECK_LAUNCH("tf_attend_plain_kernel");
    return 0;
}
