// Sampling decode for the Seq2seq recommenders (include/neuroir_sample.h).  The reference has no sampler; the semantics
// are this project's and stand at the head of the header.  A draw is the arg-max of the perturbed logits (Gumbel-max): the decode is the
// S2sStepper of csrc/seq2seq.hip (s2s_gen.hpp) over R = B N decode rows and B source rows -- the beam's row layout r = n B + b -- with a fourth
// tail behind the attentional output.  Per step, for all R rows at once:
//   (h,c) = cell(emb(tok), (h,c)); attention over source row `row % B`; o = linear_out([ctx ; h])                                 S2sStepper::step
//   per row: argmax_v fmaf(y_v, 1/tau, g_v) with its logit, and (max, sum) of exp(y), y = W_g o + b_g never written     sample_gen_kernel
//   per row: the partials merge; logp = y - lse; freeze, cum, lengths, the prediction column, the next input id         sample_finish_kernel
// or, plain form: the fp32 GEMM into workspace logits + sample_row_kernel (one workgroup per row); or, top_k > 0: nir_beam_gen_topk as it is
// (either of its forms) + sample_topk_select_kernel.  All three read the noise from ONE device function, sample_noise4: Philox4x32-10 keyed by
// the seed on the counter (v >> 2, source row, step, sample), four Gumbel values a call.  nir_sample_noise returns it to the tests.
// sample_gen_kernel is the fifth consumer of the generator tile walk, next to arg-max (s2s_gen.hpp), its STATS form, top-W (csrc/beam.hip) and
// the target logit (csrc/score.hip), and restates their staging, chunk clamp and fragment walk as they do: a change to one of those has to be
// made here too (the shared body was measured slower).
// The types, argument checks, launchers and the host-side tail other units need stand in sample_tail.hpp (SampleTail: carve, begin, draw, end --
// csrc/session_sample.hip runs the same tail behind the steps of HredQS and the session models); the kernels live here.  One decode loop,
// s2s_sample_decode, serves Seq2seq (acg == NULL: the tail's own draw) and ACG (the copy generator's draw), as s2s_decode and
// s2s_beam_decode do; SamplePlan is the only plan of this unit.  The fused walks share one launcher (launch_sample_walk) and one "take the
// partials, walk, finish" helper (sample_walk_finish); the merge loop at the head of acg_sample_row_kernel stays a copy of sample_finish_kernel's:
// factored into one device function it cost sample_finish_kernel two SGPRs.
// Everything is enqueued on the caller's stream: no host synchronisation, no allocation, no atomics, every reduction in a fixed order.
#include <cmath>
#include "s2s_gen.hpp"
#include "gen_rows.hpp"
#include "sample_tail.hpp"
#include "beam_steps.hpp"

namespace nir {

// ---- the noise: one function for every form ------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
// PRECONDITION: k0 and k1 are wave-uniform (every caller passes the seed's halves from a kernel argument): the empty asm below pins them to
// scalar registers, which holds one value per wave.  The counter words may differ per lane.
__device__ __forceinline__ void sample_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
    asm volatile("" : "+s"(k0), "+s"(k1));            // the round keys are re-derived per call on the scalar unit: hoisted, the twenty of them spill SGPRs
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// g = -log(-log u), u = ((word >> 9) + 0.5) 2^-23.  w = -log u must keep its RELATIVE accuracy -- the outer log turns it into an absolute error of
// g -- and the winners come from u -> 1, where w is tiny and a log of u itself has lost it.  So:
//   u >  1/2   w = -log1p(-q) on the exact q = 1 - u, as 2 atanh(s), s = q / (2 - q) <= 1/3: s (2 + 2 s^2 / 3 + ... + 2 s^14 / 15), the next term
//              below 2^-29 of the sum
//   u <= 1/2   w = -ln 2 log2(u): |log2 u| >= 1, where one ulp of the hardware's log2 is a relative 2^-23
// and g = -ln 2 log2(w) with the product carried in two terms (ocml's logf without its denormal and infinity branches: w lies in [2^-24, 16.7]).
// |g - g64| is measured by tests/test_gpu_sample_envelope.py against sample_ref.E_G.
__device__ __forceinline__ float sample_gumbel(uint32_t word) {
    const uint32_t m = word >> 9;
    const float u = ((float)m + 0.5f) * 0x1p-23f;
    const float q = ((float)(0x7FFFFFu - m) + 0.5f) * 0x1p-23f;                  // 1 - u, exactly
    const float s = q * __builtin_amdgcn_rcpf(2.0f - q), z = s * s;
    float a = 2.0f / 15.0f;
    a = fmaf(a, z, 2.0f / 13.0f);
    a = fmaf(a, z, 2.0f / 11.0f);
    a = fmaf(a, z, 2.0f / 9.0f);
    a = fmaf(a, z, 2.0f / 7.0f);
    a = fmaf(a, z, 2.0f / 5.0f);
    a = fmaf(a, z, 2.0f / 3.0f);
    a = fmaf(a, z, 2.0f);
    const float w = u > 0.5f ? s * a : -0x1.62e430p-1f * __log2f(u);
    const float l2 = __log2f(w), hi = l2 * 0x1.62e42ep-1f;
    return -(hi + fmaf(l2, 0x1.efa39ep-25f, fmaf(l2, 0x1.62e42ep-1f, -hi)));
}
// the Philox words and the Gumbel values of vocabulary ids 4 vq .. 4 vq + 3 for (source row b, sample n)
__device__ __forceinline__ void sample_noise4(const SampleKey& k, uint32_t vq, uint32_t b, uint32_t n, uint32_t (&word)[4], float (&g)[4]) {
    sample_philox(vq, b, k.step, n, k.k0, k.k1, word);
#pragma unroll
    for (int r = 0; r < 4; ++r) g[r] = sample_gumbel(word[r]);
}

// g [rows, VT] (and the words): one thread per (row, four ids)
__global__ __launch_bounds__(256) void sample_noise_kernel(SampleKey k, int64_t rows, int64_t VT, float* __restrict__ g, uint32_t* __restrict__ words) {
    const int64_t nq = (VT + 3) / 4;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * nq) return;
    const int64_t row = e / nq, vq = e - row * nq;
    uint32_t wd[4];
    float gv[4];
    sample_noise4(k, (uint32_t)vq, (uint32_t)(row % k.nsrc), (uint32_t)(row / k.nsrc), wd, gv);
    for (int r = 0; r < 4; ++r) {
        const int64_t v = 4 * vq + r;
        if (v < VT) {
            g[row * VT + v] = gv[r];
            if (words) words[row * VT + v] = wd[r];
        }
    }
}

// ---- where a row's choice goes ------------------------------------------------------------------------------------------------------------------
// Kernel-level entries (fin == NULL): token / logp / lse [rows], no freeze, no feedback.  Decode (fin given): the freeze rule on the row's state
// fin / cum / len [rows] (row order r = n nsrc + b), column `step` of predictions and token_logprobs [nsrc, N, max_len], and the id the next
// step reads, through lut (tgt2src), <unk> (1) outside [0, Vsrc).
// o.CV > 0 (the copy generator): ids in [VT, VT + CV) are slots of the source row's dictionary, fed back through e2s [nsrc, CV].
__device__ __forceinline__ void sample_emit(const SampleOut& o, int64_t row, int idx, float y, float lse) {
    const int tok = (idx >= 0 && (int64_t)idx < o.VT + o.CV) ? idx : 0;          // (only a row of NaN logits has no winner)
    float lp = y - lse;
    if (!o.fin) {
        o.token[row] = tok;
        o.logp[row] = lp;
        if (o.lse) o.lse[row] = lse;
        return;
    }
    int64_t t = tok;
    if (o.fin[row]) {
        t = NIR_BEAM_EOS;
        lp = 0.f;
    } else {
        o.cum[row] += lp;
        if (t == NIR_BEAM_EOS) { o.fin[row] = 1; o.len[row] = o.step + 1; }
    }
    const int64_t out = ((row % o.nsrc) * o.N + row / o.nsrc) * o.max_len + o.step;
    o.pred[out] = t;
    o.tlp[out] = lp;
    const int64_t nxt = (o.CV > 0 && t >= o.VT) ? o.e2s[(row % o.nsrc) * o.CV + (t - o.VT)] : (o.lut && t < o.VT) ? o.lut[t] : t;
    o.next_ids[row] = (nxt >= 0 && nxt < o.Vsrc) ? nxt : 1;
}

// (a, ai) in front of (b, bi): the larger perturbed value, the smaller index among equals
__device__ __forceinline__ bool sample_before(float a, int ai, float b, int bi) { return a > b || (a == b && ai < bi); }
// the best (perturbed value, index, its logit) of the wave, in every lane
__device__ __forceinline__ void sample_wave_best(float& p, int& i, float& y) {
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const float op = __shfl_xor(p, sh), oy = __shfl_xor(y, sh);
        const int oi = __shfl_xor(i, sh);
        if (sample_before(op, oi, p, i)) { p = op; i = oi; y = oy; }
    }
}

// ---- generator + bias + (perturbed arg-max, its logit, max, sum): logits[b, v] = x[b, :] . W[v, :] + bias[v] never leave the chip -------------------
// The staging, tiling, fragment format, chunked prefetch and logit expression of score_gen_target_kernel on BeamRowsF32 (the greedy kernel's
// expression: top_k = 1 and the noise-free limit pick its token).  Epilogue per lane and row tile: the online-softmax pair of the UNPERTURBED y
// (PAD substituted in the copy generator's instantiations only: the flag below), one Philox call, four Gumbel values, the perturbed compare in ascending index order ('>' keeps the
// first index on ties) carrying (perturbed best, index, that index's y).  Every wave writes one partial per decode row -- pv / pi / py / pm / ps
// [part][Bd]; a wave without tiles writes (-inf, SAMPLE_NONE, 0, -inf, 0), which the merge passes over.
// ROWSRC (gen_rows.hpp), as in beam_gen_topk_kernel: BeamRowsF32 -- fp32 rows split on load, a row block's ranges adjacent (s2s_nvr) -- or
// BeamRowsSplit -- the fp16 term pairs h16 [row][K/8][2][8] the folded LSTM step leaves (HredQS): 16-byte copies into the
// planes, hq_nvr ranges on the XCD-aware grid.  The instantiations on BeamRowsF32 compile to the registers they had before the parameter.
// PAD (the copy generator's sampler), as in beam_gen_topk_kernel<.., PAD>: the logit of v == 0 is replaced by ACG_PAD_LOGIT
// before both the online-softmax pair and the perturbed compare; the partial layout is unchanged, and acg_sample_row_kernel merges it.  PAD =
// false compiles the substitution away.
template <class ROWSRC, int NBT, bool PAD = false>
__global__ __launch_bounds__(256, 1) void sample_gen_kernel(const typename ROWSRC::elem* __restrict__ x, const _Float16* __restrict__ wfrag, const float* __restrict__ bias,
                                                            int64_t VT, int64_t ntiles, int64_t Bd, int K, int nvr, SampleKey key, float inv_tau,
                                                            float* __restrict__ pv, int* __restrict__ pi, float* __restrict__ py,
                                                            float* __restrict__ pm, float* __restrict__ ps) {
    extern __shared__ __attribute__((aligned(16))) _Float16 sample_sm[];       // [2 terms][ROWS][LD]
    constexpr int ROWS = 16 * NBT;
    const int LD = K + 8, KS = K / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g4 = lane >> 4;
    int vr;
    int64_t b0;
    ROWSRC::template map<ROWS>(nvr, Bd, vr, b0);
    const int64_t per_wg = (ntiles + nvr - 1) / nvr;
    const int64_t t_lo = (int64_t)vr * per_wg, t_hi = min(ntiles, t_lo + per_wg);
    {
        constexpr int SB = 8;                                                     // loads in flight before the first is written
        const int K4 = K / 4, total = ROWS * K4;                                  // a multiple of 256
        for (int e0 = tid; e0 < total; e0 += 256 * SB) {
            typename ROWSRC::chunk sv[SB];
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                const int e = min(e0 + 256 * q, total - 1);
                const int r = e / K4, c = e - r * K4;
                const int64_t b = b0 + r;
                sv[q] = ROWSRC::load(x, b < Bd ? b : Bd - 1, c, K);
            }
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                const int e = e0 + 256 * q;
                if (e < total) {
                    const int r = e / K4, c = e - r * K4;
                    typename ROWSRC::chunk v = sv[q];
                    if (b0 + r >= Bd) v = {};
                    ROWSRC::template store<ROWS>(sample_sm, r, c, LD, v);
                }
            }
        }
    }
    uint32_t rb[NBT], rn[NBT];                                                    // (source row, sample) of this lane's decode rows
    float best[NBT], by[NBT], rm[NBT], rs[NBT];
    int bidx[NBT];
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) {
        const uint32_t b = (uint32_t)(b0 + bt * 16 + c16);                        // Bd < 2^31
        rn[bt] = b / key.nsrc;
        rb[bt] = b - rn[bt] * key.nsrc;
        best[bt] = -INFINITY; bidx[bt] = SAMPLE_NONE; by[bt] = 0.f;
        rm[bt] = -INFINITY; rs[bt] = 0.f;
    }
    __syncthreads();
    const int NCH = (KS + GEN_KC - 1) / GEN_KC;
    const int64_t first = t_lo + wave;
    const int64_t nt = first < t_hi ? (t_hi - first + 3) / 4 : 0;             // this wave's tiles: first, first + 4, ...
    const int64_t items = nt * NCH;                                           // (tile, chunk) pairs, in order
    f32x4 acc[NBT], acx[NBT];
    auto load_w = [&](int64_t it, f16x8 (&wf)[GEN_KC][2]) {
        const int64_t t = first + 4 * (it / NCH);
        const int c = (int)(it % NCH);
#pragma unroll
        for (int u = 0; u < GEN_KC; ++u) {
            const int ks = min(c * GEN_KC + u, KS - 1);                       // clamped: a duplicate k-step is not multiplied below
            const _Float16* wp = wfrag + ((t * KS + ks) * 2 * 64 + lane) * 8;
            wf[u][0] = *reinterpret_cast<const f16x8*>(wp);
            wf[u][1] = *reinterpret_cast<const f16x8*>(wp + 512);
        }
    };
    const _Float16* bp0 = sample_sm + c16 * LD + 8 * g4;
    auto compute = [&](int64_t it, const f16x8 (&wf)[GEN_KC][2]) {
        const int64_t t = first + 4 * (it / NCH);
        const int c = (int)(it % NCH);
        if (c == 0) {
#pragma unroll
            for (int bt = 0; bt < NBT; ++bt) { acc[bt] = (f32x4){0.f, 0.f, 0.f, 0.f}; acx[bt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        }
#pragma unroll
        for (int u = 0; u < GEN_KC; ++u) {
            const int ks = c * GEN_KC + u;
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
            const int64_t v0 = t * 16 + 4 * g4;
            float bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) bv[r] = (bias && v0 + r < VT) ? bias[v0 + r] : 0.f;
#pragma unroll
            for (int bt = 0; bt < NBT; ++bt) {
                float y[4];
                float m = rm[bt];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    y[r] = fmaf(acx[bt][r], SPLIT2_INV, acc[bt][r]) + bv[r];  // the greedy, top-k and scoring kernels' expression
                    if constexpr (PAD) {
                        if (v0 + r == 0) y[r] = ACG_PAD_LOGIT;                // the reference assigns this constant behind the linear
                    }
                    if (v0 + r >= VT) y[r] = -INFINITY;                       // padded tile rows: never win, add exp(-inf) = 0
                    m = fmaxf(m, y[r]);
                }
                if (m > -INFINITY) {
                    rs[bt] = rs[bt] * __expf(rm[bt] - m) + ((__expf(y[0] - m) + __expf(y[1] - m)) + (__expf(y[2] - m) + __expf(y[3] - m)));
                    rm[bt] = m;
                }
                uint32_t wd[4];
                float g[4];
                sample_noise4(key, (uint32_t)(v0 >> 2), rb[bt], rn[bt], wd, g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {                                 // ascending in r: '>' keeps the first index on ties
                    const float p = fmaf(y[r], inv_tau, g[r]);                // (-inf for a padded row: inv_tau > 0)
                    if (p > best[bt]) { best[bt] = p; bidx[bt] = (int)(v0 + r); by[bt] = y[r]; }
                }
            }
        }
    };
    {
        f16x8 wfA[GEN_KC][2], wfB[GEN_KC][2];
        if (items > 0) load_w(0, wfA);
        for (int64_t it = 0; it < items; it += 2) {
            if (it + 1 < items) load_w(it + 1, wfB);
            compute(it, wfA);
            if (it + 1 >= items) break;
            if (it + 2 < items) load_w(it + 2, wfA);
            compute(it + 1, wfB);
        }
    }
    // lanes l, l + 16, l + 32, l + 48 hold the same decode row: the pairs combine, the smaller index wins ties; only the g4 == 0 lane's value is
    // written
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) {
#pragma unroll
        for (int sh = 16; sh <= 32; sh <<= 1) {
            const float om = __shfl_xor(rm[bt], sh), os = __shfl_xor(rs[bt], sh);
            const float m = fmaxf(om, rm[bt]);
            rs[bt] = m > -INFINITY ? rs[bt] * __expf(rm[bt] - m) + os * __expf(om - m) : 0.f;
            rm[bt] = m;
            const float op = __shfl_xor(best[bt], sh), oy = __shfl_xor(by[bt], sh);
            const int oi = __shfl_xor(bidx[bt], sh);
            if (sample_before(op, oi, best[bt], bidx[bt])) { best[bt] = op; bidx[bt] = oi; by[bt] = oy; }
        }
        const int64_t b = b0 + bt * 16 + c16;
        if (g4 == 0 && b < Bd) {
            const int64_t slot = ((int64_t)vr * 4 + wave) * Bd + b;
            pv[slot] = best[bt];
            pi[slot] = bidx[bt];
            py[slot] = by[bt];
            pm[slot] = rm[bt];
            ps[slot] = rs[bt];
        }
    }
}

// ---- the partials of one row -> (token, logp) and the tail: one wave per row, four rows a workgroup ------------------------------------------------------
// Lane l takes parts l, l + 64, ... in order; the pairs combine through wave_max / wave_sum (a fixed tree), the candidates by comparisons alone
// (ties in the perturbed value go to the smaller index, so the order of the parts does not enter).
__global__ __launch_bounds__(256) void sample_finish_kernel(const float* __restrict__ pv, const int* __restrict__ pi, const float* __restrict__ py,
                                                            const float* __restrict__ pm, const float* __restrict__ ps, int nparts, int64_t rows,
                                                            SampleOut o) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                                  // wave-uniform
    float m = -INFINITY, s = 0.f, bp = -INFINITY, byv = 0.f;
    int bi = SAMPLE_NONE;
    for (int p = lane; p < nparts; p += 64) {
        const int64_t slot = (int64_t)p * rows + row;
        const float om = pm[slot], os = ps[slot];
        const float nm = fmaxf(m, om);
        if (nm > -INFINITY) s = s * expf(m - nm) + os * expf(om - nm);
        m = nm;
        const float cp = pv[slot];
        const int ci = pi[slot];
        if (sample_before(cp, ci, bp, bi)) { bp = cp; bi = ci; byv = py[slot]; }
    }
    const float M = wave_max(m);
    const float S = wave_sum(m > -INFINITY ? s * expf(m - M) : 0.f);
    sample_wave_best(bp, bi, byv);
    if (lane == 0) sample_emit(o, row, bi, byv, M + logf(S));
}

// ---- plain form: one workgroup per row of [rows, VT] logits -> the same choice from the same noise -----------------------------------------------------------
// A thread takes the ids 4 (tid + 256 i) .. + 3: one Philox call for four logits, as in the fused kernel.
// PAD (the copy generator's sampler): logits[row, 0] is read as ACG_PAD_LOGIT and the row's choice is not emitted -- it comes out as ONE partial
// (perturbed best, its index, its logit, max, sum) in the fused kernel's layout, SamplePartials [rows], which acg_sample_row_kernel merges.
struct SamplePartials {                               // one partial per row, the fused kernel's layout
    float* pv;
    int* pi;
    float *py, *pm, *ps;
};
template <bool PAD> struct SampleRowDest { using type = SampleOut; };
template <> struct SampleRowDest<true> { using type = SamplePartials; };
template <bool PAD = false>
__global__ __launch_bounds__(256) void sample_row_kernel(const float* __restrict__ logits, int64_t VT, SampleKey key, float inv_tau,
                                                         typename SampleRowDest<PAD>::type o) {
    __shared__ float lm[4], ls[4], lp[4], ly[4];
    __shared__ int li[4];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const float* y = logits + row * VT;
    const uint32_t rn = (uint32_t)row / key.nsrc, rb = (uint32_t)row - rn * key.nsrc;
    float m = -INFINITY, s = 0.f, bp = -INFINITY, byv = 0.f;
    int bi = SAMPLE_NONE;
    for (int64_t v0 = 4 * (int64_t)tid; v0 < VT; v0 += 1024) {
        uint32_t wd[4];
        float g[4];
        sample_noise4(key, (uint32_t)(v0 >> 2), rb, rn, wd, g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                         // ascending: '>' keeps the first index on ties
            if (v0 + r < VT) {
                float a = y[v0 + r];
                if constexpr (PAD) {
                    if (v0 + r == 0) a = ACG_PAD_LOGIT;
                }
                const float nm = fmaxf(m, a);
                if (nm > -INFINITY) s = s * expf(m - nm) + expf(a - nm);
                m = nm;
                const float p = fmaf(a, inv_tau, g[r]);
                if (p > bp) { bp = p; bi = (int)(v0 + r); byv = a; }
            }
        }
    }
    const float wm = wave_max(m);
    const float wsum = wave_sum(m > -INFINITY ? s * expf(m - wm) : 0.f);
    sample_wave_best(bp, bi, byv);
    if ((tid & 63) == 0) { lm[tid >> 6] = wm; ls[tid >> 6] = wsum; lp[tid >> 6] = bp; li[tid >> 6] = bi; ly[tid >> 6] = byv; }
    __syncthreads();
    if (tid == 0) {
        const float M = fmaxf(fmaxf(lm[0], lm[1]), fmaxf(lm[2], lm[3]));
        float S = 0.f;
        for (int w = 0; w < 4; ++w) S += lm[w] > -INFINITY ? ls[w] * expf(lm[w] - M) : 0.f;
        for (int w = 1; w < 4; ++w)
            if (sample_before(lp[w], li[w], bp, bi)) { bp = lp[w]; bi = li[w]; byv = ly[w]; }
        if constexpr (PAD) {
            o.pv[row] = bp; o.pi[row] = bi; o.py[row] = byv; o.pm[row] = M; o.ps[row] = S;
        } else {
            sample_emit(o, row, bi, byv, M + logf(S));
        }
    }
}

// ---- top-k form: the choice among a row's W largest logits, perturbed by the noise of their ids: one thread per row -------------------------------------------
__global__ __launch_bounds__(256) void sample_topk_select_kernel(const float* __restrict__ top_val, const int* __restrict__ top_idx,
                                                                 const float* __restrict__ lse, int64_t rows, int W, SampleKey key, float inv_tau,
                                                                 SampleOut o) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const uint32_t rn = (uint32_t)row / key.nsrc, rb = (uint32_t)row - rn * key.nsrc;
    float bp = -INFINITY, byv = 0.f;
    int bi = SAMPLE_NONE;
    for (int j = 0; j < W; ++j) {
        const int v = top_idx[row * W + j];
        if (v < 0 || (int64_t)v >= o.VT + o.CV) continue;                     // an empty list slot
        const float a = top_val[row * W + j];
        uint32_t wd[4];
        float g[4];
        sample_noise4(key, (uint32_t)v >> 2, rb, rn, wd, g);
        const int r = v & 3;
        const float p = fmaf(a, inv_tau, r == 0 ? g[0] : r == 1 ? g[1] : r == 2 ? g[2] : g[3]);
        if (sample_before(p, v, bp, bi)) { bp = p; bi = v; byv = a; }
    }
    sample_emit(o, row, bi, byv, lse ? lse[row] : 0.f);                       // lse NULL: the lists hold log-probabilities (the copy generator's)
}

// ---- the copy generator's sampler (include/neuroir_acg_sample.h): one wave per decode row r = n nsrc + b --------------------------
// A draw from the row's COLLAPSED extended distribution, which is never written.  Steps 1-3 are those of acg_select_kernel / acg_beam_row_kernel in
// their fp32 expressions: the partials of the PAD-substituting walk merge to (m, Z) and the raw perturbed winner (its perturbed value, id and
// logit); z = sigmoid(x), 1 - z = sigmoid(-x); the copy mass of every slot (j ascending; map entries at j >= len are never read) and the slots'
// targets in LDS.  The maps, ext2tgt and the length are those of source row b; o and the copy attention are the decode row's own.  Candidates, each
// perturbed by the noise of its EXTENDED id e (counter (e >> 2, b, t, n), word e & 3):
//   the raw perturbed winner v, unless a slot collapses onto it   fmaf(l[v], 1/tau, g[v]) + c_row,  c_row = (log(1 - z) - m - log Z) / tau
//   a slot that is not collapsed                                  fmaf(logf(mass[c]), 1/tau, g[VT + c])
//   a target t of one or more slots, once                         fmaf(logf((1 - z) exp(l[t] - m) / Z + the slots' mass), 1/tau, g[t])
//                                                                 (l[t]: the fp32 row dot behind the fused walk, the GEMM's logit in the plain form)
// Among the words no slot collapses onto the perturbed values differ from the walk's by the row constant c_row alone, so their best is the walk's
// winner; if that winner is a target its exact value is at least the raw one and still dominates them.  -inf (P = 0) is never chosen; a row
// without a candidate of positive probability emits id 0.  The wave's arg-max takes the smaller id among equals; lane 0 runs the tail with
// logp = logf(P(token)), the probability at tau = 1.  No atomics; every reduction in a fixed order.
__device__ __forceinline__ float sample_noise1(const SampleKey& k, uint32_t e, uint32_t b, uint32_t n) {
    uint32_t wd[4];
    float g[4];
    sample_noise4(k, e >> 2, b, n, wd, g);
    const uint32_t r = e & 3;
    return r == 0 ? g[0] : r == 1 ? g[1] : r == 2 ? g[2] : g[3];
}
__global__ __launch_bounds__(64) void acg_sample_row_kernel(const float* __restrict__ o, int K, const float* __restrict__ gen_w, const float* __restrict__ gen_b,
                                                            int64_t VT, const float* __restrict__ pv, const int* __restrict__ pi,
                                                            const float* __restrict__ py, const float* __restrict__ pm, const float* __restrict__ ps,
                                                            int nparts, int64_t R, SampleKey key, float inv_tau, const float* __restrict__ copy_w,
                                                            const float* __restrict__ copy_b, const float* __restrict__ attn, int64_t attn_stride,
                                                            const int64_t* __restrict__ lens, int QL, const int64_t* __restrict__ map,
                                                            const int64_t* __restrict__ e2t, int CV, float* __restrict__ stat_max,
                                                            float* __restrict__ stat_lse, const float* __restrict__ logits, SampleOut out) {
    extern __shared__ float acgs_sm[];                         // mass [CV] floats, tl [CV] ints
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const uint32_t rn = (uint32_t)r / key.nsrc, rb = (uint32_t)r - rn * key.nsrc;
    const int64_t b = rb;
    float* mass = acgs_sm;
    int* tl = reinterpret_cast<int*>(acgs_sm + CV);
    // 1. the generator's statistics and the raw perturbed winner (sample_finish_kernel's merge)
    float m = -INFINITY, s = 0.f, wp = -INFINITY, wy = 0.f;
    int wi = SAMPLE_NONE;
    for (int p = lane; p < nparts; p += 64) {
        const int64_t slot = (int64_t)p * R + r;
        const float om = pm[slot], os = ps[slot];
        const float nm = fmaxf(m, om);
        if (nm > -INFINITY) s = s * expf(m - nm) + os * expf(om - nm);
        m = nm;
        const float cp = pv[slot];
        const int ci = pi[slot];
        if (sample_before(cp, ci, wp, wi)) { wp = cp; wi = ci; wy = py[slot]; }
    }
    const float M = wave_max(m);
    const float Z = wave_sum(m > -INFINITY ? s * expf(m - M) : 0.f);
    sample_wave_best(wp, wi, wy);
    if (lane == 0) {
        if (stat_max) stat_max[r] = M;
        if (stat_lse) stat_lse[r] = M + logf(Z);
    }
    // 2. the copy switch
    const float* ob = o + r * K;
    float x = 0.f;
    for (int k = 4 * lane; k < K; k += 256) {
        const float4 a = *reinterpret_cast<const float4*>(ob + k), w = *reinterpret_cast<const float4*>(copy_w + k);
        x += (a.x * w.x + a.y * w.y) + (a.z * w.z + a.w * w.w);
    }
    x = wave_sum(x) + copy_b[0];
    const float z = 1.0f / (1.0f + expf(-x)), omz = 1.0f / (1.0f + expf(x));
    // 3. the copy mass and the target of every slot of source row b
    int len = (int)lens[b];
    len = len < 0 ? 0 : (len > QL ? QL : len);
    const int64_t* mb = map + b * QL;
    const float* ab = attn + r * attn_stride;
    for (int c = lane; c < CV; c += 64) {
        float acc = 0.f;
        for (int j = 0; j < len; ++j)
            if (mb[j] == c) acc += z * ab[j];
        mass[c] = acc;
        const int64_t t = e2t[b * CV + c];
        tl[c] = (c >= 2 && t >= 0 && t < VT) ? (int)t : -1;
    }
    __syncthreads();                                           // (one wave: the LDS writes above are visible below)
    // 4. the candidates: (perturbed value, extended id, P)
    float bp = -INFINITY, bP = 0.f;
    int be = SAMPLE_NONE;
    auto take = [&](float p, int e, float P) {
        if (p > -INFINITY && sample_before(p, e, bp, be)) { bp = p; be = e; bP = P; }
    };
    auto offer = [&](float P, int e) { take(fmaf(logf(P), inv_tau, sample_noise1(key, (uint32_t)e, rb, rn)), e, P); };
    for (int c = lane; c < CV; c += 64)
        if (tl[c] < 0) offer(mass[c], (int)(VT + c));
    if (wi >= 0 && wi < VT) {                                  // wave-uniform: the raw winner, dropped when it is a target
        int hit = 0;
        for (int c = lane; c < CV; c += 64) hit |= tl[c] == wi;
        if (!__any(hit) && lane == 0) take(wp + (logf(omz) - M - logf(Z)) * inv_tau, wi, omz * expf(wy - M) / Z);
    }
    for (int c = 2; c < CV; ++c) {                             // wave-uniform: every slot that is the FIRST of its target id
        const int t = tl[c];
        if (t < 0) continue;
        int dup = 0;
        float cp = 0.f;
        for (int c2 = lane; c2 < CV; c2 += 64)
            if (tl[c2] == t) {
                if (c2 < c) dup = 1;
                else cp += mass[c2];
            }
        if (__any(dup)) continue;
        cp = wave_sum(cp);
        float lt = ACG_PAD_LOGIT;
        if (t != 0 && logits) {                                // plain form: the GEMM's own logit, the sum m and Z were formed from
            lt = logits[r * VT + t];
        } else if (t != 0) {
            const float* wr = gen_w + (int64_t)t * K;
            float d = 0.f;
            for (int k = 4 * lane; k < K; k += 256) {
                const float4 a = *reinterpret_cast<const float4*>(ob + k), w = *reinterpret_cast<const float4*>(wr + k);
                d += (a.x * w.x + a.y * w.y) + (a.z * w.z + a.w * w.w);
            }
            lt = wave_sum(d) + (gen_b ? gen_b[t] : 0.f);
        }
        if (lane == 0) offer(omz * expf(lt - M) / Z + cp, t);
    }
    sample_wave_best(bp, be, bP);
    if (lane == 0) sample_emit(out, r, be, logf(bP), 0.f);
}

// ---- the decode's first and last launch --------------------------------------------------------------------------------------------------------------
__global__ void sample_init_kernel(float* __restrict__ cum, int* __restrict__ fin, int64_t* __restrict__ len, int64_t n, int max_len) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    cum[e] = 0.f;
    fin[e] = 0;
    len[e] = max_len;
}
// one wave per decode row r = n B + b -> output (b, n): the score, the length and the attention rows of every step, attn_ws [max_len][R][QL]
__global__ __launch_bounds__(64) void sample_end_kernel(const float* __restrict__ cum, const int64_t* __restrict__ len, const float* __restrict__ attn_ws,
                                                        int64_t B, int N, int max_len, int QL, float* __restrict__ scores,
                                                        int64_t* __restrict__ lengths, float* __restrict__ attn) {
    const int64_t r = blockIdx.x, R = B * N;
    const int64_t out = (r % B) * N + r / B;
    const int lane = threadIdx.x;
    if (lane == 0) { scores[out] = cum[r]; lengths[out] = len[r]; }
    if (QL <= 0 || !attn) return;                                             // the decoders without attention output (section 29)
    for (int t = 0; t < max_len; ++t) {
        const float* ar = attn_ws + ((int64_t)t * R + r) * QL;
        float* ao = attn + (out * max_len + t) * QL;
        for (int q = lane; q < QL; q += 64) ao[q] = ar[q];
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------------------
// partials per row of the fused walk, the two policies: fp32 rows -- one per wave of every vocabulary range of s2s_nvr, a row block's ranges
// adjacent; the split state -- of hq_nvr's grid (one workgroup per CU, XCD-aware)
static int sample_nparts(int64_t rows, int K, int64_t VT) { return rows > 0 ? 4 * s2s_nvr(rows, K, (VT + 15) / 16) : 0; }
static int sample_split_nparts(int64_t rows, int K, int64_t VT) {
    return rows > 0 ? 4 * hq_nvr((rows + 16 * gen_nbt(K) - 1) / (16 * gen_nbt(K)), (VT + 15) / 16) : 0;
}
size_t sample_gen_bytes(int64_t rows, int K, int64_t VT, bool fused) {
    if (!fused) return (size_t)rows * VT * sizeof(float) + 256;
    return (size_t)sample_nparts(rows, K, VT) * rows * 5 * sizeof(float) + 5 * 256;
}
size_t sample_gen_split_bytes(int64_t rows, int K, int64_t VT) { return (size_t)sample_split_nparts(rows, K, VT) * rows * 5 * sizeof(float) + 5 * 256; }

static SamplePartials sample_take_partials(Workspace& a, size_t n) {
    SamplePartials p;
    p.pv = a.take<float>(n);
    p.pi = a.take<int>(n);
    p.py = a.take<float>(n);
    p.pm = a.take<float>(n);
    p.ps = a.take<float>(n);
    return p;
}
// the fused walk over nvr vocabulary ranges x the row blocks: 4 nvr partials a row into p, under `name` (PAD: the copy generator's instantiations)
template <class ROWSRC, bool PAD>
static int launch_sample_walk(const char* name, const typename ROWSRC::elem* x, int64_t rows, int K, int nvr, const float* gen_b, const void* gen_frag,
                              int64_t VT, const SampleKey& key, float inv_tau, const SamplePartials& p, hipStream_t st) {
    const int64_t ntiles = (VT + 15) / 16;
    const int nbt = gen_nbt(K);
    const int64_t rb = (rows + 16 * nbt - 1) / (16 * nbt);
    {
        ProfScope ps_(prof_shape_name(name, (long long)rows, (long long)VT, K), st);
        const dim3 grid((unsigned)(nvr * rb));
        if (nbt == 4) {
            static const hipError_t raised = hipFuncSetAttribute((const void*)sample_gen_kernel<ROWSRC, 4, PAD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds(512));
            (void)raised;
            hipLaunchKernelGGL((sample_gen_kernel<ROWSRC, 4, PAD>), grid, dim3(256), gen_lds(K), st, x, (const _Float16*)gen_frag, gen_b, VT, ntiles, rows, K, nvr, key,
                               inv_tau, p.pv, p.pi, p.py, p.pm, p.ps);
        } else {
            static const hipError_t raised = hipFuncSetAttribute((const void*)sample_gen_kernel<ROWSRC, 2, PAD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds(1024));
            (void)raised;
            hipLaunchKernelGGL((sample_gen_kernel<ROWSRC, 2, PAD>), grid, dim3(256), gen_lds(K), st, x, (const _Float16*)gen_frag, gen_b, VT, ntiles, rows, K, nvr, key,
                               inv_tau, p.pv, p.pi, p.py, p.pm, p.ps);
        }
    }
    NIR_CHECK_LAUNCH(name);
    return 0;
}
// take the five partial arrays (nparts a row), walk, finish(p): sample_finish_kernel, or the copy generator's row kernel
template <class ROWSRC, bool PAD, class Finish>
static int sample_walk_finish(const char* name, Workspace& a, const typename ROWSRC::elem* x, int64_t rows, int K, int nparts, const float* gen_b,
                              const void* gen_frag, int64_t VT, const SampleKey& key, float inv_tau, hipStream_t st, Finish finish) {
    const SamplePartials p = sample_take_partials(a, (size_t)nparts * rows);
    NIR_PROPAGATE((launch_sample_walk<ROWSRC, PAD>(name, x, rows, K, nparts / 4, gen_b, gen_frag, VT, key, inv_tau, p, st)));
    return finish(p);
}
static int launch_sample_finish(const SamplePartials& p, int nparts, int64_t rows, const SampleOut& o, hipStream_t st) {
    {
        ProfScope ps_("sample_finish_kernel", st);
        hipLaunchKernelGGL(sample_finish_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, p.pv, p.pi, p.py, p.pm, p.ps, nparts, rows, o);
    }
    NIR_CHECK_LAUNCH("sample_finish_kernel");
    return 0;
}

// one sampling step over the whole vocabulary on x [rows, K]: the fused kernel + finish, or the fp32 GEMM + one workgroup per row
int launch_sample_gen(bool fused, const float* x, int64_t rows, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                             const SampleKey& key, float inv_tau, void* ws, size_t ws_bytes, const SampleOut& o, hipStream_t st) {
    Workspace a(ws, ws_bytes);
    if (!fused) {
        float* logits = a.take<float>((size_t)rows * VT);
        NIR_PROPAGATE(launch_linear(x, K, nullptr, nullptr, 0, 0, 0, gen_w, K, gen_b, nullptr, logits, VT, rows, (int)VT, K, NIR_ACT_NONE, st));
        {
            ProfScope ps_("sample_row_kernel", st);
            hipLaunchKernelGGL(sample_row_kernel<false>, dim3((unsigned)rows), dim3(256), 0, st, logits, VT, key, inv_tau, o);
        }
        NIR_CHECK_LAUNCH("sample_row_kernel");
        return 0;
    }
    const int nparts = sample_nparts(rows, K, VT);
    return sample_walk_finish<BeamRowsF32, false>("sample_gen_kernel", a, x, rows, K, nparts, gen_b, gen_frag, VT, key, inv_tau, st,
                                                  [&](const SamplePartials& p) { return launch_sample_finish(p, nparts, rows, o, st); });
}
// one sampling step over the whole vocabulary on the split state h16 [rows][K/8][2][8]: sample_gen_kernel on BeamRowsSplit + the same finish
int launch_sample_gen_split(const _Float16* h16, int64_t rows, int K, const float* gen_b, const void* gen_frag, int64_t VT, const SampleKey& key,
                            float inv_tau, void* ws, size_t ws_bytes, const SampleOut& o, hipStream_t st) {
    Workspace a(ws, ws_bytes);
    const int nparts = sample_split_nparts(rows, K, VT);
    return sample_walk_finish<BeamRowsSplit, false>("hq_sample_gen_kernel", a, h16, rows, K, nparts, gen_b, gen_frag, VT, key, inv_tau, st,
                                                    [&](const SamplePartials& p) { return launch_sample_finish(p, nparts, rows, o, st); });
}
int launch_sample_topk_select(const float* top_val, const int* top_idx, const float* lse, int64_t rows, int W, const SampleKey& key, float inv_tau,
                                     const SampleOut& o, hipStream_t st) {
    {
        ProfScope ps_("sample_topk_select_kernel", st);
        hipLaunchKernelGGL(sample_topk_select_kernel, g1(rows), dim3(256), 0, st, top_val, top_idx, lse, rows, W, key, inv_tau, o);
    }
    NIR_CHECK_LAUNCH("sample_topk_select_kernel");
    return 0;
}

int launch_sample_init(float* cum, int* fin, int64_t* len, int64_t R, int max_len, hipStream_t st) {
    hipLaunchKernelGGL(sample_init_kernel, g1(R), dim3(256), 0, st, cum, fin, len, R, max_len);
    NIR_CHECK_LAUNCH("sample_init_kernel");
    return 0;
}
int launch_sample_end(const float* cum, const int64_t* len, const float* attn_ws, int64_t B, int N, int max_len, int QL, float* scores, int64_t* lengths,
                      float* attn, hipStream_t st) {
    {
        ProfScope ps_("sample_end_kernel", st);
        hipLaunchKernelGGL(sample_end_kernel, dim3((unsigned)(B * N)), dim3(64), 0, st, cum, len, attn_ws, B, N, max_len, QL, scores, lengths, attn);
    }
    NIR_CHECK_LAUNCH("sample_end_kernel");
    return 0;
}

// ---- the copy generator's sampler: the per-row launches (include/neuroir_acg_sample.h) ------------------------------------------------------------------
static bool acg_sample_dims_ok(int QL, int CV, int64_t VT) { return acg_dims_ok(QL, CV) && VT > 0 && VT + CV < 0x7FFFFFF0LL; }
// whole-distribution form: the partials (fused: sample_nparts a row; plain: the GEMM's logits in front of one a row)
static size_t acg_sample_gen_bytes(int64_t rows, int K, int64_t VT, bool fused) {
    if (fused) return sample_gen_bytes(rows, K, VT, true);
    return align_up((size_t)rows * VT * sizeof(float), 256) + 5 * align_up((size_t)rows * sizeof(float), 256) + 256;
}
// top-k form: nir_acg_beam_gen_select's workspace in front of its lists [rows, top_k]
static size_t acg_sample_topk_bytes(int64_t rows, int K, int64_t VT, int top_k, bool fused) {
    return align_up(nir_acg_beam_gen_select_workspace_bytes(rows, K, VT, top_k, fused), 256) + 2 * align_up((size_t)rows * top_k * sizeof(float), 256) + 256;
}
struct AcgSampleIn {                                   // what a row reads besides o: the switch, the copy attention and the maps of source row r % nsrc
    const float *copy_w, *copy_b, *attn;
    int64_t attn_stride;
    const int64_t* lens;
    int QL;
    const int64_t *map, *e2t, *e2s;
    int CV;
};
// one draw per row over the whole collapsed distribution: the PAD-substituting walk (fused) or the fp32 GEMM + sample_row_kernel<true> (plain), then
// acg_sample_row_kernel
static int launch_acg_sample_gen_select(bool fused, const float* o, int64_t R, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                                        const SampleKey& key, float inv_tau, const AcgSampleIn& in, void* ws, size_t ws_bytes, float* stat_max,
                                        float* stat_lse, const SampleOut& out, hipStream_t st) {
    Workspace a(ws, ws_bytes);
    float* logits = a.take<float>(fused ? 0 : (size_t)R * VT);
    const int nparts = fused ? sample_nparts(R, K, VT) : 1;
    auto row_kernel = [&](const SamplePartials& p) {
        {
            ProfScope ps_("acg_sample_row_kernel", st);
            hipLaunchKernelGGL(acg_sample_row_kernel, dim3((unsigned)R), dim3(64), (size_t)2 * in.CV * sizeof(float), st, o, K, gen_w, gen_b, VT, p.pv, p.pi, p.py, p.pm,
                               p.ps, nparts, R, key, inv_tau, in.copy_w, in.copy_b, in.attn, in.attn_stride, in.lens, in.QL, in.map, in.e2t, in.CV, stat_max, stat_lse,
                               fused ? nullptr : logits, out);
        }
        NIR_CHECK_LAUNCH("acg_sample_row_kernel");
        return 0;
    };
    if (fused) return sample_walk_finish<BeamRowsF32, true>("acg_sample_gen_kernel", a, o, R, K, nparts, gen_b, gen_frag, VT, key, inv_tau, st, row_kernel);
    const SamplePartials p = sample_take_partials(a, (size_t)R);
    NIR_PROPAGATE(launch_linear(o, K, nullptr, nullptr, 0, 0, 0, gen_w, K, gen_b, nullptr, logits, VT, R, (int)VT, K, NIR_ACT_NONE, st));
    {
        ProfScope ps_("acg_sample_plain_row_kernel", st);
        hipLaunchKernelGGL(sample_row_kernel<true>, dim3((unsigned)R), dim3(256), 0, st, logits, VT, key, inv_tau, p);
    }
    NIR_CHECK_LAUNCH("acg_sample_plain_row_kernel");
    return row_kernel(p);
}
// one draw per row among the top_k most probable entries: acg_beam_row_kernel's lists with every row live (nir_acg_beam_gen_select's body; in the
// plain form a target's logit is read from the GEMM's logits), then
// sample_topk_select_kernel on (log P, e) with lse read as 0
static int launch_acg_sample_topk(const float* o, int64_t R, int64_t nsrc, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                                  int top_k, const SampleKey& key, float inv_tau, const AcgSampleIn& in, void* ws, size_t ws_bytes, const SampleOut& out,
                                  hipStream_t st) {
    Workspace a(ws, ws_bytes);
    const size_t nb = nir_acg_beam_gen_select_workspace_bytes(R, K, VT, top_k, gen_frag != nullptr);
    char* bw = a.take<char>(nb);
    float* tval = a.take<float>((size_t)R * top_k);
    int* tidx = a.take<int>((size_t)R * top_k);
    const int rc = acg_beam_gen_select_rows(o, R, nsrc, K, gen_w, gen_b, gen_frag, VT, top_k, in.copy_w, in.copy_b, in.attn, in.attn_stride, in.lens, in.QL,
                                            in.map, in.e2t, in.e2s, in.CV, bw, nb, tval, tidx, (nir_stream_t)st, true);
    if (rc != 0) return rc;
    return launch_sample_topk_select(tval, tidx, nullptr, R, top_k, key, inv_tau, out, st);
}

// ---- the decode of Seq2seq (acg == NULL) and of ACG ---------------------------------------------------------------------------------------------------
struct SamplePlan {
    S2sStepBufs s;                                    // the stepper's buffers, over R = B N decode rows
    SampleTail t;                                     // (ACG: its generator's workspace holds the top-k lists)
    float* attn;                                      // [max_len][R][QL] the attention rows of every step
    AcgCopyAttn ca;                                   // ACG only: a copy attention of its own
    size_t bytes;
};
// acg: 0 = Seq2seq, 1 = ACG with reuse_copy_attn, 2 = ACG with a copy attention of its own
static SamplePlan sample_plan(void* ws, size_t cap, int64_t B, int QL, int N, int top_k, int max_len, int H, int64_t VT, int attn_type, bool fused, int cell,
                              bool step16, int acg) {
    Workspace a(ws, cap);
    SamplePlan p;
    const int64_t R = B * N;
    p.s = s2s_step_bufs(a, R, B, QL, H, VT, attn_type, true, cell, step16);                 // (no logits of the stepper's: the generator's workspace below)
    if (acg)
        p.t.carve(a, R, top_k, R == 0 ? 0 : top_k > 0 ? acg_sample_topk_bytes(R, H, VT, top_k, fused) : acg_sample_gen_bytes(R, H, VT, fused), false);
    else
        p.t.carve(a, R, H, VT, top_k, fused ? SAMPLE_GEN_FUSED : SAMPLE_GEN_PLAIN);
    p.s.tgt = p.t.tgt;
    if (cell == S2S_CELL_GRU) p.s.gru = a.take<float>(gru_step_scratch_floats(R, H));
    p.attn = a.take<float>((size_t)max_len * R * QL);
    if (acg == 2) p.ca.carve(a, R, B, QL, H, attn_type);
    p.bytes = align_up(a.off, 256);
    return p;
}
static size_t sample_decode_workspace_bytes(int64_t B, int QL, int N, int top_k, int max_len, const nir_seq2seq_decoder_weights* w, int cell,
                                            const AcgDecode* acg = nullptr) {
    if (!s2s_weights_ok(w) || B < 0 || QL <= 0 || max_len <= 0 || !sample_dims_ok(N, top_k, w->VT) || B * N >= 0x7FFFFFFFLL) return 0;
    if (acg && (!acg_weights_ok(w, acg) || !acg_sample_dims_ok(QL, acg->CV, w->VT))) return 0;
    return sample_plan(nullptr, 0, B, QL, N, top_k, max_len, w->H, w->VT, w->attn_type, s2s_fused(w), cell, s2s_step16(w),
                       acg ? (acg->cw->reuse_copy_attn ? 1 : 2) : 0).bytes;
}

// The stepper of s2s_gen.hpp over N decode rows per source row, with the sampling tail behind the attentional output: Seq2seq's draw is the tail's
// own; ACG's (s2s_beam_decode's tail, DESIGN.md sections 24 and 33) is (a second attention over the R rows with nsrc = B whose query is the
// attentional output,) then one draw per row from the collapsed extended distribution, or from its top_k entries.  The state ping-pongs as in the
// greedy decode: step s writes slot s & 1 and reads the other.
static int s2s_sample_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, int N, int top_k,
                             float inv_tau, uint64_t seed, const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                             const nir_seq2seq_decoder_weights* w, void* workspace, size_t workspace_bytes, int64_t* predictions, float* token_logprobs,
                             float* scores, int64_t* lengths, float* attentions, int cell, hipStream_t st, const AcgDecode* acg = nullptr) {
    const char* name = acg ? "acg_sample_decode" : "sample_seq2seq_decode";
    NIR_REQUIRE(!acg || acg->cw, "acg_sample_decode: null copy weights");
    NIR_REQUIRE(N >= 1 && B >= 0 && B * (int64_t)N < 0x7FFFFFFFLL, "%s: N < 1 or too many decode rows", name);
    const int64_t R = B * N;
    S2sStepper s{name, w, cell, table, memory_bank, source_len, V, R, B, E, QL, st};
    NIR_PROPAGATE(s.check(dec_h, dec_c, predictions && token_logprobs && scores && lengths && attentions, bos, max_len));
    NIR_REQUIRE(sample_dims_ok(N, top_k, w->VT), "%s: top_k outside 0 .. %d or above the target vocabulary", name, NIR_BEAM_MAX_W);
    NIR_REQUIRE(sample_tau_ok(inv_tau), "%s: inv_temperature must be finite and > 0", name);
    if (acg) {
        NIR_REQUIRE(acg_weights_ok(w, acg), "acg_sample_decode: copy weights incomplete for the attention type");
        NIR_REQUIRE(acg->src_map_idx && acg->ext2tgt && acg->ext2src, "acg_sample_decode: null index tensor");
        NIR_REQUIRE(acg_sample_dims_ok(QL, acg->CV, w->VT), "acg_sample_decode: QL outside [1, 4096], CV outside [2, %d], or VT + CV too large", ACG_MAX_CV);
    }
    const int H = w->H;
    const bool fused = s.fused;
    const SamplePlan p = sample_plan(workspace, workspace_bytes, B, QL, N, top_k, max_len, H, w->VT, w->attn_type, fused, cell, s.step16,
                                     acg ? (acg->cw->reuse_copy_attn ? 1 : 2) : 0);
    if (B == 0) return 0;                                 // nothing to enqueue: no workspace is needed either
    if (!workspace || p.bytes > workspace_bytes) {
        set_error("%s: workspace too small (%zu < %zu)", name, workspace_bytes, p.bytes);
        return NIR_ERR_WORKSPACE;
    }
    const SampleTail& t = p.t;
    s.b = p.s;
    NIR_PROPAGATE(s.prepare(dec_h, bos, p.s.h16[1]));
    NIR_PROPAGATE(t.init(R, max_len, st));
    if (acg) NIR_PROPAGATE(p.ca.prepare(acg->cw, memory_bank, B, QL, H, w->attn_type, st));
    SampleOut o = t.out(predictions, token_logprobs, tgt2src, V, w->VT, B, N, max_len, acg ? acg->ext2src : nullptr, acg ? acg->CV : 0);
    const float* hp = dec_h;
    const float* cp = dec_c;
    for (int step = 0; step < max_len; ++step) {
        float* hn = p.s.h[step & 1];
        float* cn = p.s.c[step & 1];
        float* arow = p.attn + (int64_t)step * R * QL;
        NIR_PROPAGATE(s.step(hp, cp, hn, cn, p.s.h16[(step + 1) & 1], p.s.h16[step & 1], arow, QL));
        const SampleKey key = sample_key(seed, step, B);
        o.step = step;
        if (!acg) {
            NIR_PROPAGATE(t.draw(fused ? SAMPLE_GEN_FUSED : SAMPLE_GEN_PLAIN, p.s.ah, nullptr, R, H, w->gen_w, w->gen_b, w->gen_frag, w->VT, top_k, key, inv_tau, o, st));
        } else {
            const float* ca = arow;
            int64_t ca_stride = QL;
            NIR_PROPAGATE(p.ca.step(acg->cw, p.s.ah, R, B, memory_bank, source_len, QL, H, w->attn_type, &ca, &ca_stride, st));
            const AcgSampleIn in{acg->cw->copy_w, acg->cw->copy_b, ca, ca_stride, source_len, QL, acg->src_map_idx, acg->ext2tgt, acg->ext2src, acg->CV};
            if (top_k > 0)
                NIR_PROPAGATE(launch_acg_sample_topk(p.s.ah, R, B, H, w->gen_w, w->gen_b, fused ? w->gen_frag : nullptr, w->VT, top_k, key, inv_tau, in, t.gen, t.gen_bytes,
                                                     o, st));
            else
                NIR_PROPAGATE(launch_acg_sample_gen_select(fused, p.s.ah, R, H, w->gen_w, w->gen_b, w->gen_frag, w->VT, key, inv_tau, in, t.gen, t.gen_bytes, nullptr,
                                                           nullptr, o, st));
        }
        hp = hn;
        cp = cn;
    }
    return t.end(B, N, max_len, scores, lengths, st, p.attn, QL, attentions);
}

}  // namespace nir

extern "C" int nir_sample_noise(uint64_t seed, int64_t step, int64_t nsrc, int64_t rows, int64_t VT, float* g, uint32_t* words, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(g, "sample_noise: null pointer");
    NIR_REQUIRE(sample_key_ok(step, nsrc, rows), "sample_noise: step outside [0, 2^32), nsrc < 1 or rows outside [0, 2^31)");
    NIR_REQUIRE(VT > 0 && VT < 0x7FFFFFF0LL, "sample_noise: VT outside [1, 2^31 - 16)");
    if (rows == 0) return 0;
    const int64_t n = rows * ((VT + 3) / 4);
    NIR_REQUIRE((n + 255) / 256 < 0x7FFFFFFFLL, "sample_noise: rows * VT too large for one launch");
    hipLaunchKernelGGL(sample_noise_kernel, g1(n), dim3(256), 0, (hipStream_t)stream, sample_key(seed, step, nsrc), rows, VT, g, words);
    NIR_CHECK_LAUNCH("sample_noise_kernel");
    return 0;
}

extern "C" size_t nir_sample_gen_workspace_bytes(int64_t rows, int K, int64_t VT, int fused) {
    using namespace nir;
    if (rows <= 0 || rows >= 0x7FFFFFFFLL || K < 4 || K > 8192 || K % 4 || VT <= 0 || VT >= 0x7FFFFFF0LL) return 0;
    return sample_gen_bytes(rows, K, VT, fused && gen_fusable(K, VT) && !tun(g_tun.exact_f32));
}

extern "C" int nir_sample_gen(const float* x, int64_t rows, int64_t nsrc, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                              float inv_temperature, uint64_t seed, int64_t step, void* workspace, size_t workspace_bytes, int32_t* token, float* logp,
                              float* lse, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(x && gen_w && token && logp, "sample_gen: null pointer");
    NIR_REQUIRE(sample_key_ok(step, nsrc, rows), "sample_gen: step outside [0, 2^32), nsrc < 1 or rows outside [0, 2^31)");
    NIR_REQUIRE(K >= 4 && K <= 8192 && K % 4 == 0, "sample_gen: K outside [4, 8192] or no multiple of 4");
    NIR_REQUIRE(VT > 0 && VT < 0x7FFFFFF0LL, "sample_gen: VT outside [1, 2^31 - 16)");
    NIR_REQUIRE(sample_tau_ok(inv_temperature), "sample_gen: inv_temperature must be finite and > 0");
    if (rows == 0) return 0;
    const bool fused = s2s_gen_fused(gen_frag, K, VT);
    if (!workspace || workspace_bytes < sample_gen_bytes(rows, K, VT, fused)) {
        set_error("sample_gen: workspace null or too small");
        return NIR_ERR_WORKSPACE;
    }
    const SampleOut o{token, logp, lse, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, VT, nsrc, 1, 0, 1};
    return launch_sample_gen(fused, x, rows, K, gen_w, gen_b, gen_frag, VT, sample_key(seed, step, nsrc), inv_temperature, workspace, workspace_bytes, o,
                             (hipStream_t)stream);
}

extern "C" int nir_sample_topk_select(const float* top_val, const int32_t* top_idx, const float* lse, int64_t rows, int64_t nsrc, int W,
                                      float inv_temperature, uint64_t seed, int64_t step, int32_t* token, float* logp, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(top_val && top_idx && lse && token && logp, "sample_topk_select: null pointer");
    NIR_REQUIRE(sample_key_ok(step, nsrc, rows), "sample_topk_select: step outside [0, 2^32), nsrc < 1 or rows outside [0, 2^31)");
    NIR_REQUIRE(W >= 1 && W <= NIR_BEAM_MAX_W, "sample_topk_select: W outside [1, %d]", NIR_BEAM_MAX_W);
    NIR_REQUIRE(sample_tau_ok(inv_temperature), "sample_topk_select: inv_temperature must be finite and > 0");
    if (rows == 0) return 0;
    const SampleOut o{token, logp, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0x7FFFFFF0LL, nsrc, 1, 0, 1};
    return launch_sample_topk_select(top_val, top_idx, lse, rows, W, sample_key(seed, step, nsrc), inv_temperature, o, (hipStream_t)stream);
}

extern "C" size_t nir_sample_seq2seq_decode_workspace_bytes(int64_t B, int QL, int N, int top_k, int max_len, const nir_seq2seq_decoder_weights* w) {
    return nir::sample_decode_workspace_bytes(B, QL, N, top_k, max_len, w, nir::S2S_CELL_LSTM);
}
extern "C" int nir_sample_seq2seq_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL,
                                         int N, int top_k, float inv_temperature, uint64_t seed, const float* table, int64_t V, int E,
                                         const int64_t* tgt2src, int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w, void* workspace,
                                         size_t workspace_bytes, int64_t* predictions, float* token_logprobs, float* scores, int64_t* lengths,
                                         float* attentions, nir_stream_t stream) {
    return nir::s2s_sample_decode(dec_h, dec_c, memory_bank, source_len, B, QL, N, top_k, inv_temperature, seed, table, V, E, tgt2src, bos, max_len, w,
                                  workspace, workspace_bytes, predictions, token_logprobs, scores, lengths, attentions, nir::S2S_CELL_LSTM,
                                  (hipStream_t)stream);
}
extern "C" size_t nir_sample_seq2seq_gru_decode_workspace_bytes(int64_t B, int QL, int N, int top_k, int max_len, const nir_seq2seq_decoder_weights* w) {
    return nir::sample_decode_workspace_bytes(B, QL, N, top_k, max_len, w, nir::S2S_CELL_GRU);
}
extern "C" int nir_sample_seq2seq_gru_decode(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, int N, int top_k,
                                             float inv_temperature, uint64_t seed, const float* table, int64_t V, int E, const int64_t* tgt2src,
                                             int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w, void* workspace, size_t workspace_bytes,
                                             int64_t* predictions, float* token_logprobs, float* scores, int64_t* lengths, float* attentions,
                                             nir_stream_t stream) {
    return nir::s2s_sample_decode(dec_h, nullptr, memory_bank, source_len, B, QL, N, top_k, inv_temperature, seed, table, V, E, tgt2src, bos, max_len, w,
                                  workspace, workspace_bytes, predictions, token_logprobs, scores, lengths, attentions, nir::S2S_CELL_GRU,
                                  (hipStream_t)stream);
}

// ---- the copy generator's sampler (include/neuroir_acg_sample.h) ---------------------------------------------------------------------------------------
extern "C" size_t nir_acg_sample_gen_select_workspace_bytes(int64_t rows, int K, int64_t VT, int top_k, int fused) {
    using namespace nir;
    if (rows <= 0 || rows >= 0x7FFFFFFFLL || K < 4 || K > 8192 || K % 4 || VT <= 0 || VT >= 0x7FFFFFF0LL || !sample_dims_ok(1, top_k, VT)) return 0;
    const bool f = fused && gen_fusable(K, VT) && !tun(g_tun.exact_f32);
    return top_k > 0 ? acg_sample_topk_bytes(rows, K, VT, top_k, f) : acg_sample_gen_bytes(rows, K, VT, f);
}

extern "C" int nir_acg_sample_gen_select(const float* o, int64_t rows, int64_t nsrc, int K, const float* gen_w, const float* gen_b, const void* gen_frag,
                                         int64_t VT, int top_k, float inv_temperature, uint64_t seed, int64_t step, const float* copy_w,
                                         const float* copy_b, const float* copy_attn, int64_t attn_stride, const int64_t* source_len, int QL,
                                         const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src, int CV, void* workspace,
                                         size_t workspace_bytes, int32_t* token, float* logp, float* gen_max, float* gen_lse, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(o && gen_w && copy_w && copy_b && copy_attn && source_len && src_map_idx && ext2tgt && ext2src && token && logp,
                "acg_sample_gen_select: null pointer");
    NIR_REQUIRE(sample_key_ok(step, nsrc, rows) && (rows == 0 || nsrc <= rows),
                "acg_sample_gen_select: step outside [0, 2^32), nsrc outside [1, rows] or rows outside [0, 2^31)");
    NIR_REQUIRE(K >= 4 && K <= 8192 && K % 4 == 0 && attn_stride >= QL, "acg_sample_gen_select: K outside [4, 8192], no multiple of 4, or attn_stride < QL");
    NIR_REQUIRE(acg_sample_dims_ok(QL, CV, VT), "acg_sample_gen_select: QL outside [1, 4096], CV outside [2, %d], or VT + CV outside [3, 2^31 - 16)", ACG_MAX_CV);
    NIR_REQUIRE(sample_dims_ok(1, top_k, VT), "acg_sample_gen_select: top_k outside 0 .. %d or above VT", NIR_BEAM_MAX_W);
    NIR_REQUIRE(sample_tau_ok(inv_temperature), "acg_sample_gen_select: inv_temperature must be finite and > 0");
    NIR_REQUIRE(top_k == 0 || (!gen_max && !gen_lse), "acg_sample_gen_select: gen_max / gen_lse are outputs of the whole-distribution form (top_k = 0)");
    if (rows == 0) return 0;
    const bool fused = s2s_gen_fused(gen_frag, K, VT);
    const size_t need = top_k > 0 ? acg_sample_topk_bytes(rows, K, VT, top_k, fused) : acg_sample_gen_bytes(rows, K, VT, fused);
    if (!workspace || workspace_bytes < need) {
        set_error("acg_sample_gen_select: workspace null or too small");
        return NIR_ERR_WORKSPACE;
    }
    const SampleOut out{token, logp, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, VT, nsrc, 1, 0, 1, ext2src, CV};
    const AcgSampleIn in{copy_w, copy_b, copy_attn, attn_stride, source_len, QL, src_map_idx, ext2tgt, ext2src, CV};
    const SampleKey key = sample_key(seed, step, nsrc);
    if (top_k > 0)
        return launch_acg_sample_topk(o, rows, nsrc, K, gen_w, gen_b, fused ? gen_frag : nullptr, VT, top_k, key, inv_temperature, in, workspace, workspace_bytes,
                                      out, (hipStream_t)stream);
    return launch_acg_sample_gen_select(fused, o, rows, K, gen_w, gen_b, gen_frag, VT, key, inv_temperature, in, workspace, workspace_bytes, gen_max, gen_lse, out,
                                        (hipStream_t)stream);
}

extern "C" size_t nir_acg_sample_decode_workspace_bytes(int64_t B, int QL, int CV, int N, int top_k, int max_len, const nir_seq2seq_decoder_weights* w,
                                                        const nir_acg_copy_weights* cw) {
    const nir::AcgDecode g{cw, nullptr, nullptr, nullptr, CV};
    return nir::sample_decode_workspace_bytes(B, QL, N, top_k, max_len, w, nir::S2S_CELL_LSTM, &g);
}
extern "C" int nir_acg_sample_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL,
                                     const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                                     const nir_seq2seq_decoder_weights* w, const nir_acg_copy_weights* cw, const int64_t* src_map_idx,
                                     const int64_t* ext2tgt, const int64_t* ext2src, int CV, int N, int top_k, float inv_temperature, uint64_t seed,
                                     void* workspace, size_t workspace_bytes, int64_t* predictions, float* token_logprobs, float* scores, int64_t* lengths,
                                     float* attentions, nir_stream_t stream) {
    const nir::AcgDecode g{cw, src_map_idx, ext2tgt, ext2src, CV};
    return nir::s2s_sample_decode(dec_h, dec_c, memory_bank, source_len, B, QL, N, top_k, inv_temperature, seed, table, V, E, tgt2src, bos, max_len, w,
                                  workspace, workspace_bytes, predictions, token_logprobs, scores, lengths, attentions, nir::S2S_CELL_LSTM,
                                  (hipStream_t)stream, &g);
}
extern "C" size_t nir_acg_sample_gru_decode_workspace_bytes(int64_t B, int QL, int CV, int N, int top_k, int max_len, const nir_seq2seq_decoder_weights* w,
                                                            const nir_acg_copy_weights* cw) {
    const nir::AcgDecode g{cw, nullptr, nullptr, nullptr, CV};
    return nir::sample_decode_workspace_bytes(B, QL, N, top_k, max_len, w, nir::S2S_CELL_GRU, &g);
}
extern "C" int nir_acg_sample_gru_decode(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, const float* table,
                                         int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w,
                                         const nir_acg_copy_weights* cw, const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src, int CV,
                                         int N, int top_k, float inv_temperature, uint64_t seed, void* workspace, size_t workspace_bytes,
                                         int64_t* predictions, float* token_logprobs, float* scores, int64_t* lengths, float* attentions,
                                         nir_stream_t stream) {
    const nir::AcgDecode g{cw, src_map_idx, ext2tgt, ext2src, CV};
    return nir::s2s_sample_decode(dec_h, nullptr, memory_bank, source_len, B, QL, N, top_k, inv_temperature, seed, table, V, E, tgt2src, bos, max_len, w,
                                  workspace, workspace_bytes, predictions, token_logprobs, scores, lengths, attentions, nir::S2S_CELL_GRU,
                                  (hipStream_t)stream, &g);
}
