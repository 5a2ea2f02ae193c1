// Seq2seq.decode -- greedy decoding of the attention encoder-decoder (neuroir/recommender/seq2seq.py:118-195; RNNDecoder:
// decoders/decoder.py:120-177, decoders/rnn_decoder.py:19-90; GlobalAttention 'general' / 'dot' / 'mlp': modules/global_attention.py:81-211).
//
// Once per decode: the bank the scores are taken against
//   general: memq = bank W_in     (score_j = (W_in h) . m_j = h . (W_in^T m_j): one GEMM instead of one per step)
//   dot:     memq = bank
//   mlp:     memc = bank W_c^T
// Per step, for all B rows at once (there is no input feed: the LSTM reads the previous token's embedding and its own state):
//   (h,c) = LSTM(emb(tok), (h,c))                     lstm_step_kernel (folded gate rows + fp16 term pairs, or the fp32 step)
//   mlp only: qh = W_q h + b_q                        GEMM
//   a = softmax_j(mask(score_j)); ctx = sum_j a_j m_j; cat = [ctx ; h]; attentions[b, step, :] = a          s2s_attend_kernel
//   o = linear_out(cat)  (+ tanh for general / dot; + bias, no tanh for mlp)                            GEMM + epilogue
//   tok' = argmax_v (W_g o + b_g)_v; tok = lut[tok']                                                    s2s_gen_argmax_kernel + argmax_finish_kernel
//                                                                                                    (or GEMM + argmax_map_kernel)
// Everything is enqueued on the caller's stream; no host synchronisation, no allocation, no float atomics.
#include <algorithm>
#include <mutex>
#include "decode_common.hpp"

namespace nir {

// ---- attention step: one wave per decode row -----------------------------------------------------------------------------------
// q: general / dot -- the decoder state h (the scores are h . sb_j); mlp -- W_q h + b_q (the scores are sum_f v_f tanh(q_f + sb[j, f])).
// sb [B, QL, H]: the score bank (memq / bank / memc);  mem [B, QL, H]: the memory bank the context is taken from.
// cat [B, 2H] = [ctx ; h];  attn row b at attn + b * attn_stride, [QL]: masked positions get an exact 0.0 (a row of length 0 is NaN
// throughout, like the reference's softmax over an all -inf row).
__global__ __launch_bounds__(256) void s2s_attend_kernel(const float* __restrict__ q, const float* __restrict__ h, const float* __restrict__ mem,
                                                         const float* __restrict__ sb, const float* __restrict__ v,
                                                         const int64_t* __restrict__ lens, int B, int QL, int H, int mlp, float* __restrict__ cat,
                                                         float* __restrict__ attn, int64_t attn_stride) {
    extern __shared__ float s2s_pr[];                 // [4][QL]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= B) return;
    float* pw = s2s_pr + wave * QL;
    int len = (int)lens[i];
    len = len < 0 ? 0 : (len > QL ? QL : len);
    const float* mb = mem + (int64_t)i * QL * H;
    const float* sq = sb + (int64_t)i * QL * H;
    const float* qi = q + (int64_t)i * H;
    float mx = -INFINITY;
    for (int j = 0; j < len; ++j) {
        float s = 0.f;
        for (int f = 4 * lane; f < H; f += 256) {
            const float4 a = *reinterpret_cast<const float4*>(sq + (int64_t)j * H + f), b = *reinterpret_cast<const float4*>(qi + f);
            if (mlp) {
                const float4 w = *reinterpret_cast<const float4*>(v + f);
                s += (w.x * tanhf(a.x + b.x) + w.y * tanhf(a.y + b.y)) + (w.z * tanhf(a.z + b.z) + w.w * tanhf(a.w + b.w));
            } else {
                s += (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
            }
        }
        s = wave_sum(s);
        if (lane == 0) pw[j] = s;
        mx = fmaxf(mx, s);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float den = 0.f;
    for (int j = 0; j < len; ++j) den += expf(pw[j] - mx);
    float* ar = attn + (int64_t)i * attn_stride;
    for (int j = lane; j < QL; j += 64) ar[j] = len == 0 ? NAN : (j < len ? expf(pw[j] - mx) / den : 0.0f);
    float* o = cat + (int64_t)i * 2 * H;
    for (int f = 4 * lane; f < H; f += 256) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < len; ++j) {
            const float p = expf(pw[j] - mx) / den;
            const float4 x = *reinterpret_cast<const float4*>(mb + (int64_t)j * H + f);
            acc.x = fmaf(p, x.x, acc.x); acc.y = fmaf(p, x.y, acc.y); acc.z = fmaf(p, x.z, acc.z); acc.w = fmaf(p, x.w, acc.w);
        }
        if (len == 0) acc = make_float4(NAN, NAN, NAN, NAN);
        *reinterpret_cast<float4*>(o + f) = acc;
        *reinterpret_cast<float4*>(o + H + f) = *reinterpret_cast<const float4*>(h + (int64_t)i * H + f);
    }
}

// ---- generator + bias + arg-max: logits[b, v] = x[b, :] . W[v, :] + bias[v] never leave the chip --------------------------------
// W [VT, K] (K = 32 .. 1024, a multiple of 32) arrives as two fp16 term planes in MFMA A-fragment order (s2s_gen_frag_kernel):
//   frag[vt][ks][term][lane][8],  element (lane, j) = W[16 vt + (lane & 15)][32 ks + 8 (lane >> 4) + j],  rows past VT are zero.
// A workgroup stages 16 NBT decode rows as two fp16 planes in LDS ([2][16 NBT][K + 8] halves: NBT = 4 up to K = 512 -- 133 KB -- and 2
// beyond -- 132 KB at K = 1024; gfx950 has 160 KB) and walks its range of vocabulary tiles, a wave one tile at a time.  A tile's k-steps
// go in chunks of S2S_KC: the fragments of the next chunk (or of the next tile's first chunk) are requested before the MFMAs of the
// current one are issued.  Three v_mfma_f32_16x16x32_f16 per product block (hi hi -> acc; lo hi, hi lo -> acx; result acc + 2^-11 acx),
// the bias is added in fp32 before the comparison, `>` in ascending index order keeps the first index on ties.  Every wave writes one
// (value, index) partial per decode row; argmax_finish_kernel reduces them.
constexpr int S2S_KC = 8;

template <int NBT>
__global__ __launch_bounds__(256, 1) void s2s_gen_argmax_kernel(const float* __restrict__ x, const _Float16* __restrict__ wfrag,
                                                                const float* __restrict__ bias, int64_t VT, int64_t ntiles, int64_t Bd, int K,
                                                                int nvr, float* __restrict__ pval, int* __restrict__ pidx) {
    extern __shared__ __attribute__((aligned(16))) _Float16 s2s_sm[];          // [2 terms][ROWS][LD]
    constexpr int ROWS = 16 * NBT;
    const int LD = K + 8, KS = K / 32, K4 = K / 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g4 = lane >> 4;
    const int vr = (int)(blockIdx.x % nvr);
    const int64_t b0 = (int64_t)(blockIdx.x / nvr) * ROWS;
    const int64_t per_wg = (ntiles + nvr - 1) / nvr;
    const int64_t t_lo = (int64_t)vr * per_wg, t_hi = min(ntiles, t_lo + per_wg);
    {
        // stage + split this workgroup's decode rows (zero rows past Bd).  The loads of S2S_SB trips are issued before the first is converted
        // (unconditional, from a clamped element: a branch around a load puts an s_waitcnt vmcnt(0) at its join), as in pred_argmax_kernel:
        // one load -> convert -> ds_write per trip would be 4 NBT K / 256 dependent L2 round trips.
        constexpr int S2S_SB = 8;
        const int total = ROWS * K4;                                              // a multiple of 256
        for (int e0 = tid; e0 < total; e0 += 256 * S2S_SB) {
            float4 sv[S2S_SB];
#pragma unroll
            for (int q = 0; q < S2S_SB; ++q) {
                const int e = min(e0 + 256 * q, total - 1);
                const int r = e / K4, k4 = (e - r * K4) * 4;
                const int64_t b = b0 + r;
                sv[q] = *reinterpret_cast<const float4*>(x + (b < Bd ? b : Bd - 1) * K + k4);
            }
#pragma unroll
            for (int q = 0; q < S2S_SB; ++q) {
                const int e = e0 + 256 * q;
                if (e < total) {
                    const int r = e / K4, k4 = (e - r * K4) * 4;
                    float4 v = sv[q];
                    if (b0 + r >= Bd) v = make_float4(0.f, 0.f, 0.f, 0.f);
                    const Split2x4 sp = split2(v);
                    _Float16* d = s2s_sm + r * LD + k4;
                    *reinterpret_cast<uint2*>(d) = sp.hi;
                    *reinterpret_cast<uint2*>(d + ROWS * LD) = sp.lo;
                }
            }
        }
    }
    __syncthreads();
    float best[NBT];
    int bidx[NBT];
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) { best[bt] = -INFINITY; bidx[bt] = 0x7FFFFFFF; }
    const int NCH = (KS + S2S_KC - 1) / S2S_KC;
    const int64_t first = t_lo + wave;
    const int64_t nt = first < t_hi ? (t_hi - first + 3) / 4 : 0;             // this wave's tiles: first, first + 4, ...
    const int64_t items = nt * NCH;                                           // (tile, chunk) pairs, in order
    f32x4 acc[NBT], acx[NBT];
    auto load_w = [&](int64_t it, f16x8 (&wf)[S2S_KC][2]) {
        const int64_t t = first + 4 * (it / NCH);
        const int c = (int)(it % NCH);
#pragma unroll
        for (int u = 0; u < S2S_KC; ++u) {
            const int ks = min(c * S2S_KC + u, KS - 1);                       // clamped: a duplicate k-step is not multiplied below
            const _Float16* wp = wfrag + ((t * KS + ks) * 2 * 64 + lane) * 8;
            wf[u][0] = *reinterpret_cast<const f16x8*>(wp);
            wf[u][1] = *reinterpret_cast<const f16x8*>(wp + 512);
        }
    };
    const _Float16* bp0 = s2s_sm + c16 * LD + 8 * g4;
    auto compute = [&](int64_t it, const f16x8 (&wf)[S2S_KC][2]) {
        const int64_t t = first + 4 * (it / NCH);
        const int c = (int)(it % NCH);
        if (c == 0) {
#pragma unroll
            for (int bt = 0; bt < NBT; ++bt) { acc[bt] = (f32x4){0.f, 0.f, 0.f, 0.f}; acx[bt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        }
#pragma unroll
        for (int u = 0; u < S2S_KC; ++u) {
            const int ks = c * S2S_KC + u;
            if (ks < KS) {                                                    // wave-uniform
                f16x8 b[NBT][2];
#pragma unroll
                for (int bt = 0; bt < NBT; ++bt) {
                    b[bt][0] = *reinterpret_cast<const f16x8*>(bp0 + 32 * ks + bt * 16 * LD);
                    b[bt][1] = *reinterpret_cast<const f16x8*>(bp0 + 32 * ks + bt * 16 * LD + ROWS * LD);
                }
#pragma unroll
                for (int bt = 0; bt < NBT; ++bt) acx[bt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u][1], b[bt][0], acx[bt], 0, 0, 0);
#pragma unroll
                for (int bt = 0; bt < NBT; ++bt) acc[bt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u][0], b[bt][0], acc[bt], 0, 0, 0);
#pragma unroll
                for (int bt = 0; bt < NBT; ++bt) acx[bt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u][0], b[bt][1], acx[bt], 0, 0, 0);
            }
        }
        if (c == NCH - 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t v = t * 16 + 4 * g4 + r;                        // ascending in r: '>' keeps the first index on ties
                if (v < VT) {
                    const float bv = bias ? bias[v] : 0.f;
#pragma unroll
                    for (int bt = 0; bt < NBT; ++bt) {
                        const float y = fmaf(acx[bt][r], SPLIT2_INV, acc[bt][r]) + bv;
                        if (y > best[bt]) { best[bt] = y; bidx[bt] = (int)v; }
                    }
                }
            }
        }
    };
    {
        f16x8 wfA[S2S_KC][2], wfB[S2S_KC][2];
        if (items > 0) load_w(0, wfA);
        for (int64_t it = 0; it < items; it += 2) {
            if (it + 1 < items) load_w(it + 1, wfB);
            compute(it, wfA);
            if (it + 1 >= items) break;
            if (it + 2 < items) load_w(it + 2, wfA);
            compute(it + 1, wfB);
        }
    }
    // lanes l, l + 16, l + 32, l + 48 hold the same decode row: combine (first index wins ties), then one partial per wave and row
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) {
#pragma unroll
        for (int sh = 16; sh <= 32; sh <<= 1) {
            const float ov = __shfl_xor(best[bt], sh);
            const int oi = __shfl_xor(bidx[bt], sh);
            if (ov > best[bt] || (ov == best[bt] && oi < bidx[bt])) { best[bt] = ov; bidx[bt] = oi; }
        }
        const int64_t b = b0 + bt * 16 + c16;
        if (g4 == 0 && b < Bd) {
            const int64_t slot = ((int64_t)vr * 4 + wave) * Bd + b;
            pval[slot] = best[bt];
            pidx[slot] = bidx[bt];
        }
    }
}

// generator.weight [VT, K] fp32 -> the fragment order above (h1 rounded to nearest); err_flag bit 1: a weight outside the split's range
__global__ void s2s_gen_frag_kernel(const float* __restrict__ w, int64_t VT, int K, int64_t n, _Float16* __restrict__ frag, int* __restrict__ err) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // one (tile, k-step, lane, j)
    if (e >= n) return;
    const int KS = K / 32;
    const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
    const int64_t tk = e >> 9;
    const int ks = (int)(tk % KS);
    const int64_t t = tk / KS;
    const int64_t row = t * 16 + (lane & 15);
    const int col = 32 * ks + 8 * (lane >> 4) + j;
    const float v = row < VT ? w[row * K + col] : 0.f;
    if (!(fabsf(v) < 32768.f) && err) atomicOr(err, 2);
    const _Float16 a = split2_hi1_rne(v);
    _Float16* d = frag + (tk * 2 * 64 + lane) * 8 + j;
    d[0] = a;
    d[512] = split2_lo1(v, a);
}

constexpr int S2S_MAX_WGS = 256;
static inline int s2s_nbt(int K) { return K <= 512 ? 4 : 2; }
static inline size_t s2s_lds(int K) { return (size_t)2 * 16 * s2s_nbt(K) * (K + 8) * sizeof(_Float16); }
static inline bool s2s_fusable(int K, int64_t VT) { return K >= 32 && K <= 1024 && K % 32 == 0 && VT > 0 && VT < 0x7FFFFFF0LL; }

// workgroups per row block: enough for the chip, at least ~2 tiles per wave
static int s2s_nvr(int64_t Bd, int K, int64_t ntiles) {
    const int64_t rb = (Bd + 16 * s2s_nbt(K) - 1) / (16 * s2s_nbt(K));
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(S2S_MAX_WGS, (device_cu_count() + rb - 1) / rb), (ntiles + 7) / 8));
}

static int launch_gen_argmax(const float* x, const void* frag, const float* bias, int64_t VT, int64_t Bd, int K, float* pval, int* pidx,
                             const int64_t* lut, int64_t* pred, int64_t pstride, int64_t* tgt, int64_t Vsrc, hipStream_t st) {
    const int64_t ntiles = (VT + 15) / 16;
    const int nbt = s2s_nbt(K), nvr = s2s_nvr(Bd, K, ntiles);
    const int64_t rb = (Bd + 16 * nbt - 1) / (16 * nbt);
    const size_t lds = s2s_lds(K);
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute((const void*)s2s_gen_argmax_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s2s_lds(512));
        (void)hipFuncSetAttribute((const void*)s2s_gen_argmax_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s2s_lds(1024));
    });
    {
        ProfScope ps(prof_shape_name("s2s_gen_argmax_kernel", (long long)Bd, (long long)VT, K), st);
        if (nbt == 4)
            hipLaunchKernelGGL(s2s_gen_argmax_kernel<4>, dim3((unsigned)(nvr * rb)), dim3(256), lds, st, x, (const _Float16*)frag, bias, VT, ntiles, Bd, K,
                               nvr, pval, pidx);
        else
            hipLaunchKernelGGL(s2s_gen_argmax_kernel<2>, dim3((unsigned)(nvr * rb)), dim3(256), lds, st, x, (const _Float16*)frag, bias, VT, ntiles, Bd, K,
                               nvr, pval, pidx);
    }
    NIR_CHECK_LAUNCH("s2s_gen_argmax_kernel");
    return launch_argmax_finish(pval, pidx, nvr * 4, Bd, lut, pred, pstride, tgt, Vsrc, st);
}

static int launch_attend(const float* q, const float* h, const float* mem, const float* sb, const float* v, const int64_t* lens, int64_t B, int QL,
                         int H, int mlp, float* cat, float* attn, int64_t attn_stride, hipStream_t st) {
    {
        ProfScope ps("s2s_attend_kernel", st);
        hipLaunchKernelGGL(s2s_attend_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), (size_t)4 * QL * sizeof(float), st, q, h, mem, sb, v, lens, (int)B,
                           QL, H, mlp, cat, attn, attn_stride);
    }
    NIR_CHECK_LAUNCH("s2s_attend_kernel");
    return 0;
}

struct S2sPlan {
    float *sb, *h[2], *c[2], *h16[2], *qh, *cat, *ah, *logits, *pval;
    int* pidx;
    int64_t* tgt;
    size_t bytes;
};
static S2sPlan s2s_plan(void* ws, size_t cap, int64_t B, int QL, int H, int64_t VT, int attn_type, bool fused) {
    Workspace a(ws, cap);
    S2sPlan p;
    p.sb = a.take<float>(attn_type == NIR_S2S_ATTN_DOT ? 0 : (size_t)B * QL * H);
    for (int k = 0; k < 2; ++k) { p.h[k] = a.take<float>((size_t)B * H); p.c[k] = a.take<float>((size_t)B * H); }
    for (int k = 0; k < 2; ++k) p.h16[k] = a.take<float>((size_t)B * H);
    p.qh = a.take<float>(attn_type == NIR_S2S_ATTN_MLP ? (size_t)B * H : 0);
    p.cat = a.take<float>((size_t)B * 2 * H);
    p.ah = a.take<float>((size_t)B * H);
    p.logits = a.take<float>(fused ? 0 : (size_t)B * VT);
    p.pval = a.take<float>(fused ? (size_t)S2S_MAX_WGS * 4 * B : 0);
    p.pidx = a.take<int>(fused ? (size_t)S2S_MAX_WGS * 4 * B : 0);
    p.tgt = a.take<int64_t>((size_t)B);
    p.bytes = align_up(a.off, 256);
    return p;
}
static bool s2s_fused(const nir_seq2seq_decoder_weights* w) {
    return w->gen_frag != nullptr && s2s_fusable(w->H, w->VT) && !tun(g_tun.exact_f32);
}
static bool s2s_weights_ok(const nir_seq2seq_decoder_weights* w) {
    if (!w || w->H <= 0 || w->H % 4 || w->VT <= 0) return false;
    if (!(w->rnn_wih && w->rnn_whh && w->rnn_bih && w->rnn_bhh && w->attn_out_w && w->gen_w && w->gen_b)) return false;
    if (w->attn_type == NIR_S2S_ATTN_GENERAL) return w->attn_in_wt != nullptr;
    if (w->attn_type == NIR_S2S_ATTN_DOT) return true;
    if (w->attn_type == NIR_S2S_ATTN_MLP) return w->attn_ctx_w && w->attn_query_w && w->attn_query_b && w->attn_v && w->attn_out_b;
    return false;
}

}  // namespace nir

extern "C" size_t nir_seq2seq_gen_frag_bytes(int64_t VT, int K) {
    if (!nir::s2s_fusable(K, VT)) return 0;
    return (size_t)((VT + 15) / 16) * (K / 32) * 2 * 64 * 8 * sizeof(_Float16);
}

extern "C" int nir_seq2seq_pack_gen_frag(const float* gen_w, int64_t VT, int K, void* frag, int* err_flag, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(gen_w && frag, "seq2seq_pack_gen_frag: null pointer");
    NIR_REQUIRE(s2s_fusable(K, VT), "seq2seq_pack_gen_frag: K must be a multiple of 32 in [32, 1024] and 0 < VT < 2^31 - 16");
    const int64_t n = (VT + 15) / 16 * (K / 32) * 512;
    hipLaunchKernelGGL(s2s_gen_frag_kernel, g1(n), dim3(256), 0, (hipStream_t)stream, gen_w, VT, K, n, (_Float16*)frag, err_flag);
    NIR_CHECK_LAUNCH("s2s_gen_frag_kernel");
    return 0;
}

extern "C" size_t nir_seq2seq_gen_argmax_workspace_bytes(int64_t rows, int K, int64_t VT, int fused) {
    if (rows <= 0 || K <= 0 || VT <= 0) return 0;
    return fused ? (size_t)nir::S2S_MAX_WGS * 4 * rows * 8 + 512 : (size_t)rows * VT * sizeof(float) + 256;
}

extern "C" int nir_seq2seq_gen_argmax(const float* x, int64_t rows, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                                      const int64_t* tgt2src, int64_t V, void* workspace, size_t workspace_bytes, int64_t* predictions,
                                      int64_t pred_stride, int64_t* next_tokens, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(x && gen_w && predictions && next_tokens && workspace, "seq2seq_gen_argmax: null pointer");
    NIR_REQUIRE(rows >= 0 && K > 0 && K % 4 == 0 && VT > 0 && V > 0 && pred_stride >= 1, "seq2seq_gen_argmax: bad dims");
    const bool fused = gen_frag != nullptr && s2s_fusable(K, VT) && !tun(g_tun.exact_f32);
    NIR_REQUIRE(fused || VT < 0x7FFFFFFFLL, "seq2seq_gen_argmax: VT too large for the GEMM path");
    if (workspace_bytes < nir_seq2seq_gen_argmax_workspace_bytes(rows, K, VT, fused)) {
        set_error("seq2seq_gen_argmax: workspace too small");
        return NIR_ERR_WORKSPACE;
    }
    if (rows == 0) return 0;
    Workspace a(workspace, workspace_bytes);
    if (fused) {
        float* pval = a.take<float>((size_t)S2S_MAX_WGS * 4 * rows);
        int* pidx = a.take<int>((size_t)S2S_MAX_WGS * 4 * rows);
        return launch_gen_argmax(x, gen_frag, gen_b, VT, rows, K, pval, pidx, tgt2src, predictions, pred_stride, next_tokens, V, st);
    }
    float* logits = a.take<float>((size_t)rows * VT);
    NIR_PROPAGATE(launch_linear(x, K, nullptr, nullptr, 0, 0, 0, gen_w, K, gen_b, nullptr, logits, VT, rows, (int)VT, K, NIR_ACT_NONE, st));
    return launch_argmax_map(logits, VT, tgt2src, predictions, pred_stride, next_tokens, V, rows, st);
}

extern "C" int nir_seq2seq_attend(const float* q, const float* h, const float* memory_bank, const float* score_bank, const float* v,
                                  const int64_t* source_len, int64_t B, int QL, int H, int attn_type, float* cat, float* attn,
                                  int64_t attn_stride, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(q && h && memory_bank && score_bank && source_len && cat && attn, "seq2seq_attend: null pointer");
    NIR_REQUIRE(B >= 0 && QL > 0 && QL <= 4096 && H > 0 && H % 4 == 0 && attn_stride >= QL, "seq2seq_attend: bad dims");
    NIR_REQUIRE(attn_type == NIR_S2S_ATTN_GENERAL || attn_type == NIR_S2S_ATTN_DOT || attn_type == NIR_S2S_ATTN_MLP, "seq2seq_attend: attention type");
    NIR_REQUIRE(attn_type != NIR_S2S_ATTN_MLP || v, "seq2seq_attend: mlp attention needs v");
    if (B == 0) return 0;
    return launch_attend(q, h, memory_bank, score_bank, v, source_len, B, QL, H, attn_type == NIR_S2S_ATTN_MLP, cat, attn, attn_stride,
                         (hipStream_t)stream);
}

extern "C" size_t nir_seq2seq_decode_workspace_bytes(int64_t B, int QL, const nir_seq2seq_decoder_weights* w) {
    if (!nir::s2s_weights_ok(w) || B < 0 || QL <= 0) return 0;
    return nir::s2s_plan(nullptr, 0, B, QL, w->H, w->VT, w->attn_type, nir::s2s_fused(w)).bytes;
}

extern "C" int nir_seq2seq_decode_greedy(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B,
                                         int QL, const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                                         const nir_seq2seq_decoder_weights* w, void* workspace, size_t workspace_bytes, int64_t* predictions,
                                         float* attentions, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(dec_h && dec_c && memory_bank && source_len && table && w && predictions && attentions, "seq2seq_decode: null pointer");
    NIR_REQUIRE(s2s_weights_ok(w), "seq2seq_decode: decoder weights incomplete for the attention type, or H not a multiple of 4");
    NIR_REQUIRE(B >= 0 && QL > 0 && QL <= 4096 && max_len > 0 && V > 0 && E > 0 && E % 4 == 0, "seq2seq_decode: bad dims");
    NIR_REQUIRE(bos >= 0 && bos < V, "seq2seq_decode: BOS id outside the vocabulary");
    NIR_REQUIRE((w->rnn_gate_fold == nullptr) == (w->rnn_whh_frag == nullptr), "seq2seq_decode: rnn_gate_fold and rnn_whh_frag come together");
    const int H = w->H;
    const bool fused = s2s_fused(w);
    NIR_REQUIRE(fused || w->VT < 0x7FFFFFFFLL, "seq2seq_decode: VT too large for the GEMM path");
    S2sPlan p = s2s_plan(workspace, workspace_bytes, B, QL, H, w->VT, w->attn_type, fused);
    if (!workspace || p.bytes > workspace_bytes) {
        set_error("seq2seq_decode: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
        return NIR_ERR_WORKSPACE;
    }
    if (B == 0) return 0;
    const bool mlp = w->attn_type == NIR_S2S_ATTN_MLP;
    const float* sb = memory_bank;
    if (w->attn_type == NIR_S2S_ATTN_GENERAL) {          // memq = bank W_in  (global_attention.py:98-105)
        NIR_PROPAGATE(launch_linear(memory_bank, H, nullptr, nullptr, 0, 0, 0, w->attn_in_wt, H, nullptr, nullptr, p.sb, H, B * QL, H, H, NIR_ACT_NONE, st));
        sb = p.sb;
    } else if (mlp) {                                     // memc = linear_context(bank)  (global_attention.py:112-114)
        NIR_PROPAGATE(launch_linear(memory_bank, H, nullptr, nullptr, 0, 0, 0, w->attn_ctx_w, H, nullptr, nullptr, p.sb, H, B * QL, H, H, NIR_ACT_NONE, st));
        sb = p.sb;
    }
    NIR_PROPAGATE(launch_fill_i64(p.tgt, bos, B, st));
    LstmStepArgs a;
    a.x[0] = table; a.xid[0] = p.tgt; a.xstride[0] = E;
    a.wih[0] = w->rnn_wih; a.whh[0] = w->rnn_whh; a.bih[0] = w->rnn_bih; a.bhh[0] = w->rnn_bhh;
    a.x[1] = nullptr; a.xid[1] = nullptr; a.xstride[1] = 0; a.wih[1] = a.whh[1] = a.bih[1] = a.bhh[1] = nullptr;
    a.hprev[1] = a.cprev[1] = nullptr; a.hnext[1] = a.cnext[1] = nullptr;
    a.chain0 = 0; a.B = (int)B; a.I = E; a.H = H;
    const bool step16 = w->rnn_gate_fold && w->rnn_whh_frag && H % 32 == 0 && !tun(g_tun.exact_f32);
    if (step16) {
        a.gx[0] = w->rnn_gate_fold; a.gxid[0] = p.tgt; a.gxstride = (int64_t)4 * H; a.gx_unit_major = 1;
        a.whh_frag[0] = w->rnn_whh_frag;
        NIR_PROPAGATE(launch_h16_pack(dec_h, B * H, reinterpret_cast<_Float16*>(p.h16[1]), st));
    }
    const float* hp = dec_h;
    const float* cp = dec_c;
    for (int step = 0; step < max_len; ++step) {
        float* hn = p.h[step & 1];
        float* cn = p.c[step & 1];
        a.hprev[0] = hp; a.cprev[0] = cp; a.hnext[0] = hn; a.cnext[0] = cn;
        if (step16) {
            a.h16prev[0] = reinterpret_cast<const _Float16*>(p.h16[(step + 1) & 1]);
            a.h16next[0] = reinterpret_cast<_Float16*>(p.h16[step & 1]);
        }
        NIR_PROPAGATE(launch_lstm_step(a, 1, st));
        if (mlp)
            NIR_PROPAGATE(launch_linear(hn, H, nullptr, nullptr, 0, 0, 0, w->attn_query_w, H, w->attn_query_b, nullptr, p.qh, H, B, H, H, NIR_ACT_NONE, st));
        NIR_PROPAGATE(launch_attend(mlp ? p.qh : hn, hn, memory_bank, sb, w->attn_v, source_len, B, QL, H, mlp, p.cat, attentions + (int64_t)step * QL,
                                    (int64_t)max_len * QL, st));
        NIR_PROPAGATE(launch_linear(p.cat, 2 * H, nullptr, nullptr, 0, 0, 0, w->attn_out_w, 2 * H, mlp ? w->attn_out_b : nullptr, nullptr, p.ah, H, B, H,
                                    2 * H, mlp ? NIR_ACT_NONE : NIR_ACT_TANH, st));
        if (fused) {
            NIR_PROPAGATE(launch_gen_argmax(p.ah, w->gen_frag, w->gen_b, w->VT, B, H, p.pval, p.pidx, tgt2src, predictions + step, (int64_t)max_len, p.tgt,
                                            V, st));
        } else {
            NIR_PROPAGATE(launch_linear(p.ah, H, nullptr, nullptr, 0, 0, 0, w->gen_w, H, w->gen_b, nullptr, p.logits, w->VT, B, (int)w->VT, H, NIR_ACT_NONE, st));
            NIR_PROPAGATE(launch_argmax_map(p.logits, w->VT, tgt2src, predictions + step, (int64_t)max_len, p.tgt, V, B, st));
        }
        hp = hn;
        cp = cn;
    }
    return 0;
}
