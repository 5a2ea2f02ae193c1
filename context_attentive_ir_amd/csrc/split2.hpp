// Shared by the matrix-core kernels: the vector types, the two-term fp16 split of an fp32 operand, the in-place
// v_mfma_f32_16x16x32_f16 forms and the packed LSTM cell.
#pragma once
#include "common.hpp"

namespace nir {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 fp16x2_t __attribute__((ext_vector_type(2)));      // what v_cvt_pkrtz_f16_f32 returns

// ---------------------------------------------------------------------------------------------------------------------
// The split2 format: an fp32 value x (operands bounded by 2^15, e.g. tanh / sigmoid outputs, embeddings, weights) is carried as two
// fp16 terms, x = h1 + 2^-11 h2' with
//     h1  = fp16(x)               round-toward-zero where the value is split in a kernel's hot path: v_cvt_pkrtz_f16_f32 converts AND packs
//                                 two values per instruction.  The weight-packing kernels round h1 to nearest; either way the residual
//                                 x - h1 is exact in fp32
//     h2' = fp16(2^11 (x - h1))   the residual, scaled by 2^11 (SPLIT2_SCALE) so that it does not sink into fp16's subnormals: h1 keeps
//                                 11 mantissa bits, h2' the next 11.
// A product block is three v_mfma_f32_16x16x32_f16: the leading product h1 h1 goes to one accumulator set (acc), the two cross terms
// h2' h1 and h1 h2' (both scaled by 2^11) to a second one (acx); the result is acc + 2^-11 acx (split2_combine).  That is 3 fp16 MFMAs
// per k-block instead of the 6 bf16 ones of the three-term split (common.hpp: split3), ~4 VALU ops per element instead of 5.5, 2 LDS
// planes instead of 3, at fp32-class accuracy (the dropped h2' h2' term is 2^-22 relative).
// Lower range: h2' is an fp16 subnormal (quantum 2^-24) once 2^11 |x - h1| < 2^-14, so x is carried to max(2^-22 |x|, 2^-35) absolute:
// fp32-class down to |x| ~ 2^-13, then the relative precision falls off (operands of 2^-20: about 3e-5 of a GEMM result).
// Range: |x| < 2^15, else h1 overflows fp16.  Kernels that pack caller-provided weights test !(|w| < 32768) per element and raise bit 1
// (value 2) of their error flag; the entry points that split activations on the fly take a host-checked `bounded` promise instead.
// The helpers return values; where the terms go (LDS plane, fragment order, global) is the call site's business.  hipcc's schedule
// follows statement order: split2() packs pair by pair; a site that wants another order composes split2_hi / split2_res itself.
// ---------------------------------------------------------------------------------------------------------------------
constexpr float SPLIT2_SCALE = 2048.0f, SPLIT2_INV = 1.0f / 2048.0f;

__device__ __forceinline__ fp16x2_t split2_hi(float x, float y) { return __builtin_amdgcn_cvt_pkrtz(x, y); }       // h1 of two values (rtz)
template <typename H>
__device__ __forceinline__ float split2_res(float x, H h) { return (x - (float)h) * SPLIT2_SCALE; }              // 2^11 (x - h1), fp32
__device__ __forceinline__ unsigned split2_word(fp16x2_t a) { return __builtin_bit_cast(unsigned, a); }
__device__ __forceinline__ uint2 split2_words(fp16x2_t a, fp16x2_t b) { return make_uint2(split2_word(a), split2_word(b)); }
__device__ __forceinline__ float split2_combine(float acc, float acx) { return fmaf(acx, SPLIT2_INV, acc); }
__device__ __forceinline__ f32x4 split2_combine(f32x4 acc, f32x4 acx) { return acx * SPLIT2_INV + acc; }

// one value at a time (weight packing, recurrent state): h1 rounded toward zero / to nearest, and h2' for either
__device__ __forceinline__ _Float16 split2_hi1_rtz(float x) { return (_Float16)split2_hi(x, 0.f)[0]; }
__device__ __forceinline__ _Float16 split2_hi1_rne(float x) { return (_Float16)x; }
__device__ __forceinline__ _Float16 split2_lo1(float x, _Float16 h) { return (_Float16)split2_res(x, h); }

struct Split2x2 { fp16x2_t hi, lo; };                         // two values: one 32-bit word per term
struct Split2x4 { uint2 hi, lo; };                            // four values: one 8-byte store per term
__device__ __forceinline__ Split2x2 split2(float x, float y) {
    const fp16x2_t h = split2_hi(x, y);
    return {h, split2_hi(split2_res(x, h[0]), split2_res(y, h[1]))};
}
__device__ __forceinline__ Split2x4 split2(const float4& v) {
    const fp16x2_t a01 = split2_hi(v.x, v.y), a23 = split2_hi(v.z, v.w);
    const fp16x2_t b01 = split2_hi(split2_res(v.x, a01[0]), split2_res(v.y, a01[1]));
    const fp16x2_t b23 = split2_hi(split2_res(v.z, a23[0]), split2_res(v.w, a23[1]));
    return {split2_words(a01, a23), split2_words(b01, b23)};
}

// In-place accumulate in AGPRs (MMA_A) or VGPRs (MMA_V).  Written as inline assembly: with the builtin, hipcc assigns the result of each
// accumulator chain to a different register tuple than its loop-carried input and rotates most tuples through VGPRs on every k-step
// (112 v_accvgpr_* moves per 60 MFMAs).  The operands come straight from ds_read / global_load (s_waitcnt is still compiler-inserted);
// the accumulators are first read by VALU code after MMA_DRAIN.
#define MMA_A(ACC, A, W) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(ACC) : "v"(A), "v"(W))
#define MMA_V(ACC, A, W) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(ACC) : "v"(A), "v"(W))
// first product of an accumulator chain: C = 0 (no zero fill of the accumulator registers between two GEMMs)
#define MMA0_A(ACC, A, W) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=a"(ACC) : "v"(A), "v"(W))
#define MMA0_V(ACC, A, W) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=v"(ACC) : "v"(A), "v"(W))
#define MMA_DRAIN() asm volatile("s_nop 15\n\ts_nop 15" ::: "memory")

// MFMA number n of a k-step (n is a compile-time constant after unrolling): column tile n / (3 RT), term pair (n / RT) % 3, row tile n % RT
template <int CT, int RT>
__device__ __forceinline__ void mma_n(int n, f32x4 (&acc)[CT][RT], f32x4 (&acx)[CT][RT], const f16x8 (&af)[RT][2], const f16x8 (&w)[CT][2]) {
    const int j = n / (3 * RT), ph = (n / RT) % 3, i = n % RT;
    if (ph == 0) MMA_A(acx[j][i], af[i][1], w[j][0]);
    else if (ph == 1) MMA_A(acx[j][i], af[i][0], w[j][1]);
    else MMA_A(acc[j][i], af[i][0], w[j][0]);
}

// LSTM cell on the four pre-activations x = (i, f, g, o) of one unit, merged fractions: sigma(i) tanh(g) = sgn(g) (1 - d) / ((1 + a)(1 + d))
// with a = e^-i, d = e^-2|g| (d in (0, 1]; a = inf gives 1 / inf = 0, the right limit), likewise o and tanh(c): 5 v_exp_f32 + 3 v_rcp_f32
// instead of 5 + 5 -- the transcendentals are quarter rate, and the VALU port (gate math of all waves of a SIMD) is as loaded as the
// matrix pipe in these recurrences.  The plain arithmetic is packed along the gate axis, (i, f) and (g, o) are adjacent accumulator
// registers: v_pk_{fma,mul,add}_f32 without any register shuffling.
__device__ __forceinline__ void lstm_cell_v(const f32x4 x, float& c, float& h) {
    constexpr float L2E = 1.4426950408889634f;
    const f32x2 e_if = (f32x2){x[0], x[1]} * (f32x2){-L2E, -L2E};
    const f32x2 e_go = (f32x2){fabsf(x[2]), x[3]} * (f32x2){-2.f * L2E, -L2E};
    const float a = __builtin_amdgcn_exp2f(e_if.x), b = __builtin_amdgcn_exp2f(e_if.y);
    const float d = __builtin_amdgcn_exp2f(e_go.x), q = __builtin_amdgcn_exp2f(e_go.y);
    const f32x2 p_ab = (f32x2){a, b} + (f32x2){1.f, 1.f};
    const f32x2 p_dq = (f32x2){d, q} + (f32x2){1.f, 1.f};
    const float r1 = __builtin_amdgcn_rcpf(p_ab.x * p_dq.x), rf = __builtin_amdgcn_rcpf(p_ab.y);
    c = fmaf(c, rf, copysignf((1.f - d) * r1, x[2]));
    const float e = __builtin_amdgcn_exp2f(fabsf(c) * (-2.f * L2E));
    h = copysignf((1.f - e) * __builtin_amdgcn_rcpf(p_dq.y * (1.f + e)), c);
}

// The same cell for N units at once, written statement by statement ACROSS the units: program order is then N independent dependence chains
// interleaved (every instruction's operand was produced N instructions earlier), which is what an in-order wave needs when this block is
// issued between the MFMAs of another sequence group -- unit by unit, each v_exp / v_rcp result was consumed by the very next instruction.
template <int N>
__device__ __forceinline__ void lstm_cell_vn(const f32x4 (&x)[N], float (&c)[N], float (&h)[N]) {
    constexpr float L2E = 1.4426950408889634f;
    f32x2 e_if[N], e_go[N], p_ab[N], p_dq[N];
    float a[N], b[N], d[N], q[N], r1[N], rf[N], e[N], t1[N], t2[N];
#pragma unroll
    for (int i = 0; i < N; ++i) e_if[i] = (f32x2){x[i][0], x[i][1]} * (f32x2){-L2E, -L2E};
#pragma unroll
    for (int i = 0; i < N; ++i) e_go[i] = (f32x2){fabsf(x[i][2]), x[i][3]} * (f32x2){-2.f * L2E, -L2E};
#pragma unroll
    for (int i = 0; i < N; ++i) a[i] = __builtin_amdgcn_exp2f(e_if[i].x);
#pragma unroll
    for (int i = 0; i < N; ++i) b[i] = __builtin_amdgcn_exp2f(e_if[i].y);
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] = __builtin_amdgcn_exp2f(e_go[i].x);
#pragma unroll
    for (int i = 0; i < N; ++i) q[i] = __builtin_amdgcn_exp2f(e_go[i].y);
#pragma unroll
    for (int i = 0; i < N; ++i) p_ab[i] = (f32x2){a[i], b[i]} + (f32x2){1.f, 1.f};
#pragma unroll
    for (int i = 0; i < N; ++i) p_dq[i] = (f32x2){d[i], q[i]} + (f32x2){1.f, 1.f};
#pragma unroll
    for (int i = 0; i < N; ++i) t1[i] = p_ab[i].x * p_dq[i].x;
#pragma unroll
    for (int i = 0; i < N; ++i) r1[i] = __builtin_amdgcn_rcpf(t1[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) rf[i] = __builtin_amdgcn_rcpf(p_ab[i].y);
#pragma unroll
    for (int i = 0; i < N; ++i) t2[i] = (1.f - d[i]) * r1[i];
#pragma unroll
    for (int i = 0; i < N; ++i) c[i] = fmaf(c[i], rf[i], copysignf(t2[i], x[i][2]));
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = __builtin_amdgcn_exp2f(fabsf(c[i]) * (-2.f * L2E));
#pragma unroll
    for (int i = 0; i < N; ++i) t1[i] = p_dq[i].y * (1.f + e[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) r1[i] = __builtin_amdgcn_rcpf(t1[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) h[i] = copysignf((1.f - e[i]) * r1[i], c[i]);
}

}  // namespace nir
