// Teacher-forced scoring of candidate queries (include/neuroir_score.h): log P(target[r] | x[r]) for ALL decoder rows of a
// call at once -- B N (TL - 1) of them, tens of thousands -- with the generator's logits y = W_g x + b_g never written.
//   per row: (max, sum) of exp(y) per wave and the target's biased logit                                       score_gen_target_kernel
//   per row: the partials merge to lse; logp = y[target] - lse, masked (PAD, id outside the vocabulary)         score_finish_kernel
//   per sequence: the sum and the count of the positions in front of and at the first EOS                      score_sequences_kernel
// The plain form (no fragments, a K the fused kernel does not take, tunable exact_f32) runs the fp32 GEMM into a bounded logits buffer, row
// chunk by row chunk, and score_row_kernel (one workgroup per row) behind it.
// score_gen_target_kernel is the fourth consumer of the generator tile walk, next to arg-max (s2s_gen.hpp), its STATS form and top-W
// (csrc/beam.hip), and restates their staging, chunk clamp and fragment walk as they do: a change to one of those has to be made here too.
// The rows and the grid mapping are BeamRowsF32's (gen_rows.hpp); what differs from the per-step kernels is the number of vocabulary ranges
// (score_nvr): with hundreds of row blocks the chip is full whatever the split, and a range is made long so that a row block is staged seldom.
// The copy generator's scorer (include/neuroir_acg_score.h) lives here too, so that the tile walk is not restated a fifth
// time: the PADSUB form of score_gen_target_kernel, a resolve kernel in front (extended id -> word / slot) and acg_score_finish_kernel behind.
// Everything is enqueued on the caller's stream: no host synchronisation, no allocation, no float atomics, every reduction in a fixed order.
#include "decode_common.hpp"
#include "gen_rows.hpp"
#include "s2s_gen.hpp"

namespace nir {

constexpr int64_t SCORE_ROW_CHUNK = (int64_t)1 << 18;           // rows a launch: bounds every grid and the partials
constexpr size_t SCORE_PLAIN_LOGITS_BYTES = (size_t)256 << 20;  // the plain form's logits buffer (one row where a row is larger)
constexpr int64_t SCORE_STAGE_TILES = 12;                       // what staging a row block costs, in vocabulary tiles of one workgroup (measured)

// Vocabulary ranges of score_gen_target_kernel over nrb row blocks.  A workgroup fills a CU (the staged rows take its LDS), so the grid runs in
// ceil(nrb n / CUs) rounds, and a workgroup costs its staging -- SCORE_STAGE_TILES tiles' worth, whatever K: both scale with it -- plus its
// ceil(ntiles / n) tiles: the n with the smallest product, the smallest such n, at least ~2 tiles a wave.  With hundreds of row blocks that is
// a handful of long ranges (2 at 380 row blocks on 256 CUs: three full rounds), with a few row blocks enough ranges to fill the chip once
// (13 at 19).  The model's order of the candidates is the measured one.
static inline int score_nvr(int64_t nrb, int64_t ntiles) {
    const int64_t cu = device_cu_count(), cap = std::max<int64_t>(1, std::min<int64_t>(S2S_MAX_WGS, (ntiles + 7) / 8));
    int64_t best = 1, best_cost = INT64_MAX;
    for (int64_t n = 1; n <= cap; ++n) {
        const int64_t cost = ((nrb * n + cu - 1) / cu) * (SCORE_STAGE_TILES + (ntiles + n - 1) / n);
        if (cost < best_cost) best = n, best_cost = cost;
    }
    return (int)best;
}

// ---- generator + bias + (max, sum, the target's logit) ------------------------------------------------------------------------------------------
// The staging, tiling, fragment format, chunked prefetch and logit expression of beam_gen_topk_kernel on BeamRowsF32.  Every lane keeps, per
// batch tile, the online-softmax pair (max, sum) and the target id of its decode row (staged once per row block: -1 outside [0, VT), which no
// vocabulary index equals); the one lane of the grid that computes element (row, target[row]) stores the biased logit into tlogit[row] -- a
// plain store, one owner per row, none for a target out of range.  Every wave writes one (max, sum) partial per decode row, pm / ps
// [part][Bd]; a wave without tiles writes (-inf, 0), which the merge passes over.
// PADSUB (the copy generator's scorer, include/neuroir_acg_score.h): the biased logit of v == 0 is replaced by ACG_PAD_LOGIT
// before it enters (max, sum) and before the target compare, as PAD does in beam_gen_topk_kernel; a row whose word is PAD stores the substituted
// value.  TG: the type of the per-row word ids (that scorer resolves its extended ids into int32 words once per call).  PADSUB = false compiles
// to the kernel without the test.
template <int NBT, bool PADSUB = false, typename TG = int64_t>
__global__ __launch_bounds__(256, 1) void score_gen_target_kernel(const float* __restrict__ x, const _Float16* __restrict__ wfrag,
                                                                  const float* __restrict__ bias, int64_t VT, int64_t ntiles, int64_t Bd, int K, int nvr,
                                                                  const TG* __restrict__ target, float* __restrict__ tlogit,
                                                                  float* __restrict__ pm, float* __restrict__ ps) {
    extern __shared__ __attribute__((aligned(16))) _Float16 score_sm[];        // [2 terms][ROWS][LD]
    constexpr int ROWS = 16 * NBT;
    const int LD = K + 8, KS = K / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g4 = lane >> 4;
    int vr;
    int64_t b0;
    BeamRowsF32::map<ROWS>(nvr, Bd, vr, b0);
    const int64_t per_wg = (ntiles + nvr - 1) / nvr;
    const int64_t t_lo = (int64_t)vr * per_wg, t_hi = min(ntiles, t_lo + per_wg);
    {
        constexpr int SB = 8;                                                     // loads in flight before the first is written
        const int K4 = K / 4, total = ROWS * K4;                                  // a multiple of 256
        for (int e0 = tid; e0 < total; e0 += 256 * SB) {
            float4 sv[SB];
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                const int e = min(e0 + 256 * q, total - 1);
                const int r = e / K4, c = e - r * K4;
                const int64_t b = b0 + r;
                sv[q] = BeamRowsF32::load(x, b < Bd ? b : Bd - 1, c, K);
            }
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                const int e = e0 + 256 * q;
                if (e < total) {
                    const int r = e / K4, c = e - r * K4;
                    float4 v = sv[q];
                    if (b0 + r >= Bd) v = {};
                    BeamRowsF32::store<ROWS>(score_sm, r, c, LD, v);
                }
            }
        }
    }
    int tg[NBT];
    float rm[NBT], rs[NBT];
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) {
        const int64_t b = b0 + bt * 16 + c16;
        const int64_t t = target[b < Bd ? b : Bd - 1];
        tg[bt] = (b < Bd && t >= 0 && t < VT) ? (int)t : -1;
        rm[bt] = -INFINITY;
        rs[bt] = 0.f;
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
    const _Float16* bp0 = score_sm + c16 * LD + 8 * g4;
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
                    y[r] = fmaf(acx[bt][r], SPLIT2_INV, acc[bt][r]) + bv[r];  // the greedy and top-k kernels' expression
                    if constexpr (PADSUB) {
                        if (v0 + r == 0) y[r] = ACG_PAD_LOGIT;                // the reference assigns this constant behind the linear
                    }
                    if (v0 + r >= VT) y[r] = -INFINITY;                       // padded tile rows: add exp(-inf) = 0
                    m = fmaxf(m, y[r]);
                }
                if (m > -INFINITY) {
                    rs[bt] = rs[bt] * __expf(rm[bt] - m) + ((__expf(y[0] - m) + __expf(y[1] - m)) + (__expf(y[2] - m) + __expf(y[3] - m)));
                    rm[bt] = m;
                }
                const int d = tg[bt] - (int)v0;                               // tg = -1 never lands in [0, 4): v0 >= 0
                if (d >= 0 && d < 4) tlogit[b0 + bt * 16 + c16] = d == 0 ? y[0] : d == 1 ? y[1] : d == 2 ? y[2] : y[3];
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
    // lanes l, l + 16, l + 32, l + 48 hold the same decode row: the pairs combine; only the g4 == 0 lane's value is written
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) {
#pragma unroll
        for (int sh = 16; sh <= 32; sh <<= 1) {
            const float om = __shfl_xor(rm[bt], sh), os = __shfl_xor(rs[bt], sh);
            const float m = fmaxf(om, rm[bt]);
            rs[bt] = m > -INFINITY ? rs[bt] * __expf(rm[bt] - m) + os * __expf(om - m) : 0.f;
            rm[bt] = m;
        }
        const int64_t b = b0 + bt * 16 + c16;
        if (g4 == 0 && b < Bd) {
            const int64_t slot = ((int64_t)vr * 4 + wave) * Bd + b;
            pm[slot] = rm[bt];
            ps[slot] = rs[bt];
        }
    }
}

// the masked log-probability of one row from its lse and -- where the target lies inside the vocabulary -- the target's logit
__device__ __forceinline__ void score_write_row(int64_t row, float l, float tl, bool ok, bool pad_target, float* __restrict__ token_logp,
                                                float* __restrict__ lse, int* __restrict__ id_flag) {
    if (!ok && id_flag) atomicOr(id_flag, 1);
    token_logp[row] = (ok && !pad_target) ? tl - l : 0.f;
    if (lse) lse[row] = l;
}

// ---- the partials of one row -> lse -> the masked log-probability: one wave per row, four rows a workgroup ------------------------------------------
// pm / ps [nparts][rows]; lane l takes parts l, l + 64, ... in order, the wave combines through wave_max / wave_sum (a fixed tree).  token_logp[row]
// holds the target's logit on entry where the target is inside the vocabulary (score_gen_target_kernel's tlogit) and the result on exit.
__global__ __launch_bounds__(256) void score_finish_kernel(const float* __restrict__ pm, const float* __restrict__ ps, int nparts, int64_t rows,
                                                           const int64_t* __restrict__ target, int64_t pad, int64_t VT, float* __restrict__ token_logp,
                                                           float* __restrict__ lse, int* __restrict__ id_flag) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                                  // wave-uniform
    float m = -INFINITY, s = 0.f;
    for (int p = lane; p < nparts; p += 64) {
        const int64_t slot = (int64_t)p * rows + row;
        const float om = pm[slot], os = ps[slot];
        const float nm = fmaxf(m, om);
        if (nm > -INFINITY) s = s * expf(m - nm) + os * expf(om - nm);
        m = nm;
    }
    const float M = wave_max(m);
    const float S = wave_sum(m > -INFINITY ? s * expf(m - M) : 0.f);
    if (lane == 0) {
        const int64_t t = target[row];
        const bool ok = t >= 0 && t < VT;
        score_write_row(row, M + logf(S), ok ? token_logp[row] : 0.f, ok, t == pad, token_logp, lse, id_flag);
    }
}

// ---- plain form: one workgroup per row of [rows, VT] logits -> the same (lse, target logit) ------------------------------------------------------------
__global__ __launch_bounds__(256) void score_row_kernel(const float* __restrict__ logits, int64_t VT, const int64_t* __restrict__ target, int64_t pad,
                                                        float* __restrict__ token_logp, float* __restrict__ lse, int* __restrict__ id_flag) {
    __shared__ float lm[4], ls[4];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const float* y = logits + row * VT;
    float m = -INFINITY, s = 0.f;
    for (int64_t v = tid; v < VT; v += 256) {
        const float a = y[v];
        const float nm = fmaxf(m, a);
        if (nm > -INFINITY) s = s * expf(m - nm) + expf(a - nm);
        m = nm;
    }
    const float wm = wave_max(m);
    const float wsum = wave_sum(m > -INFINITY ? s * expf(m - wm) : 0.f);
    if ((tid & 63) == 0) { lm[tid >> 6] = wm; ls[tid >> 6] = wsum; }
    __syncthreads();
    if (tid == 0) {
        const float M = fmaxf(fmaxf(lm[0], lm[1]), fmaxf(lm[2], lm[3]));
        float S = 0.f;
        for (int w = 0; w < 4; ++w) S += lm[w] > -INFINITY ? ls[w] * expf(lm[w] - M) : 0.f;
        const int64_t t = target[row];
        const bool ok = t >= 0 && t < VT;
        score_write_row(row, M + logf(S), ok ? y[t] : 0.f, ok, t == pad, token_logp, lse, id_flag);
    }
}

// ---- sequences: one thread per sequence, positions in order ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void score_sequences_kernel(float* __restrict__ token_logp, const int64_t* __restrict__ target, int64_t nseq, int T,
                                                              int64_t pad, int64_t eos, float* __restrict__ scores, int64_t* __restrict__ lengths) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nseq) return;
    float* lp = token_logp + q * T;
    const int64_t* tg = target + q * T;
    float sum = 0.f;
    int64_t n = 0;
    bool ended = false;
    for (int j = 0; j < T; ++j) {
        const int64_t t = tg[j];
        if (!ended && t != pad && t >= 0) {
            sum += lp[j];
            ++n;
        } else {
            lp[j] = 0.f;
        }
        ended = ended || (eos >= 0 && t == eos);
    }
    scores[q] = sum;
    lengths[q] = n;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------------------------
static int64_t score_nrb(int64_t rows, int K) { return (rows + 16 * gen_nbt(K) - 1) / (16 * gen_nbt(K)); }
static int score_nparts(int64_t rows, int K, int64_t VT) { return 4 * score_nvr(score_nrb(rows, K), (VT + 15) / 16); }
static size_t score_chunk_bytes(int64_t rows, int K, int64_t VT) { return (size_t)score_nparts(rows, K, VT) * rows * 2 * sizeof(float) + 2 * 256; }
// the fused form's workspace: the partials of the largest chunk -- the full one, or the short last one with more ranges over fewer row blocks
static size_t score_fused_bytes(int64_t rows, int K, int64_t VT) {
    const int64_t full = std::min(rows, SCORE_ROW_CHUNK), last = rows % SCORE_ROW_CHUNK;
    return std::max(score_chunk_bytes(full, K, VT), last ? score_chunk_bytes(last, K, VT) : 0);
}
static int64_t score_plain_rows(int64_t VT) { return std::max<int64_t>(1, (int64_t)(SCORE_PLAIN_LOGITS_BYTES / ((size_t)VT * sizeof(float)))); }
static size_t score_plain_bytes(int64_t rows, int64_t VT) { return (size_t)std::min(rows, score_plain_rows(VT)) * VT * sizeof(float) + 256; }

// the launch of score_gen_target_kernel<NBT, PADSUB, TG> over `rows` rows (one chunk): the row blocks, the vocabulary ranges, the LDS size and its
// raised limit are stated here once, for the generator's scorer and for the copy generator's.  pm / ps hold 4 nvr parts of `rows` floats each.
template <bool PADSUB, typename TG>
static void launch_score_gen_walk(const char* name, const float* x, const void* frag, const float* bias, int64_t VT, int64_t rows, int K, int nvr,
                                  const TG* target, float* tlogit, float* pm, float* ps, hipStream_t st) {
    const int64_t nrb = score_nrb(rows, K), ntiles = (VT + 15) / 16;
    ProfScope ps_(prof_shape_name(name, (long long)rows, (long long)VT, K), st);
    const dim3 grid((unsigned)(nrb * nvr));                                   // nrb <= 2^18 / 32, nvr <= S2S_MAX_WGS
    if (gen_nbt(K) == 4) {
        static const hipError_t raised =
            hipFuncSetAttribute((const void*)score_gen_target_kernel<4, PADSUB, TG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds(512));
        (void)raised;
        hipLaunchKernelGGL((score_gen_target_kernel<4, PADSUB, TG>), grid, dim3(256), gen_lds(K), st, x, (const _Float16*)frag, bias, VT, ntiles, rows, K,
                           nvr, target, tlogit, pm, ps);
    } else {
        static const hipError_t raised =
            hipFuncSetAttribute((const void*)score_gen_target_kernel<2, PADSUB, TG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds(1024));
        (void)raised;
        hipLaunchKernelGGL((score_gen_target_kernel<2, PADSUB, TG>), grid, dim3(256), gen_lds(K), st, x, (const _Float16*)frag, bias, VT, ntiles, rows, K,
                           nvr, target, tlogit, pm, ps);
    }
}

static int launch_score_gen_target(const float* x, const void* frag, const float* bias, int64_t VT, int64_t rows, int K, const int64_t* target, int64_t pad,
                                   void* ws, size_t ws_bytes, float* token_logp, float* lse, int* id_flag, hipStream_t st) {
    const int nvr = score_nvr(score_nrb(rows, K), (VT + 15) / 16), nparts = 4 * nvr;
    Workspace a(ws, ws_bytes);
    float* pm = a.take<float>((size_t)nparts * rows);
    float* ps = a.take<float>((size_t)nparts * rows);
    launch_score_gen_walk<false, int64_t>("score_gen_target_kernel", x, frag, bias, VT, rows, K, nvr, target, token_logp, pm, ps, st);
    NIR_CHECK_LAUNCH("score_gen_target_kernel");
    {
        ProfScope ps_("score_finish_kernel", st);
        hipLaunchKernelGGL(score_finish_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, pm, ps, nparts, rows, target, pad, VT, token_logp, lse,
                           id_flag);
    }
    NIR_CHECK_LAUNCH("score_finish_kernel");
    return 0;
}

// ---- the copy generator's scorer (include/neuroir_acg_score.h) -----------------------------------------------------------------
// log P of a given EXTENDED id under the collapsed extended distribution of nir_acg_beam_gen_select, per teacher-forced row, with neither the
// [rows, VT] logits nor a [rows, CV] copy distribution written.
//   once per call: extended id -> (generator word or -1, slot or -1 / masked), int32                              acg_score_resolve_kernel
//   per row: (max, sum) per wave and the word's logit, PAD substituted: score_gen_target_kernel<.., PADSUB>  |  acg_score_row_kernel (plain form)
//   per row: merge, the copy switch, the copy mass of the row's word or slot, log P, mask                         acg_score_finish_kernel
constexpr int ACG_SCORE_MASKED = -2;                            // slot[r]: the row reads 0 (PAD, or an id outside [0, VT + CV))

// Row r of the call reads source row r / rows_per_src.  word[r]: the generator column that enters P (the id itself below VT, the collapse target
// of a slot c >= 2 with ext2tgt in [0, VT)), -1 for a slot that is not collapsed and for a masked row -- which score_gen_target_kernel takes as
// "no target".  slot[r]: c for such a slot, -1 for a word, ACG_SCORE_MASKED for a masked row.  An id at or past VT + CV ORs bit 0 into id_flag;
// a negative one does not.
__global__ __launch_bounds__(256) void acg_score_resolve_kernel(const int64_t* __restrict__ target, int64_t rows, int64_t rows_per_src, int64_t VT, int CV,
                                                                const int64_t* __restrict__ e2t, int64_t pad, int* __restrict__ word,
                                                                int* __restrict__ slot, int* __restrict__ id_flag) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int64_t e = target[r];
    int w = -1, s = ACG_SCORE_MASKED;
    if (e >= VT + CV) {
        if (id_flag) atomicOr(id_flag, 1);
    } else if (e >= 0 && e != pad) {
        if (e < VT) {
            w = (int)e;
            s = -1;
        } else {
            const int c = (int)(e - VT);
            const int64_t t = e2t[(r / rows_per_src) * CV + c];
            if (c >= 2 && t >= 0 && t < VT) {                  // one word has one probability, however it is spelled
                w = (int)t;
                s = -1;
            } else {
                s = c;
            }
        }
    }
    word[r] = w;
    slot[r] = s;
}

// plain form: one workgroup per row of [rows, VT] logits -> the row's (max, sum) as ONE partial and the word's logit, logits[row, 0] read as
// ACG_PAD_LOGIT (score_row_kernel's reduction with beam_row_topk_kernel<PAD>'s override)
__global__ __launch_bounds__(256) void acg_score_row_kernel(const float* __restrict__ logits, int64_t VT, const int* __restrict__ word,
                                                            float* __restrict__ tlogit, float* __restrict__ pm, float* __restrict__ ps) {
    __shared__ float lm[4], ls[4];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const float* y = logits + row * VT;
    float m = -INFINITY, s = 0.f;
    for (int64_t v = tid; v < VT; v += 256) {
        const float a = v == 0 ? ACG_PAD_LOGIT : y[v];
        const float nm = fmaxf(m, a);
        if (nm > -INFINITY) s = s * expf(m - nm) + expf(a - nm);
        m = nm;
    }
    const float wm = wave_max(m);
    const float wsum = wave_sum(m > -INFINITY ? s * expf(m - wm) : 0.f);
    if ((tid & 63) == 0) { lm[tid >> 6] = wm; ls[tid >> 6] = wsum; }
    __syncthreads();
    if (tid == 0) {
        const float M = fmaxf(fmaxf(lm[0], lm[1]), fmaxf(lm[2], lm[3]));
        float S = 0.f;
        for (int w = 0; w < 4; ++w) S += lm[w] > -INFINITY ? ls[w] * expf(lm[w] - M) : 0.f;
        pm[row] = M;
        ps[row] = S;
        const int t = word[row];
        if (t >= 0) tlogit[row] = t == 0 ? ACG_PAD_LOGIT : y[t];
    }
}

// One wave per row, four rows a workgroup.  pm / ps [nparts][rows] as in score_finish_kernel; token_logp[row] holds the word's logit on entry
// where word[row] >= 0 and the result on exit.  The switch and the copy mass are acg_beam_row_kernel's fp32 expressions: x by the same wave dot,
// z = 1 / (1 + exp(-x)) and 1 - z = 1 / (1 + exp(x)), and the mass a sum of z a[j] in ascending j over the positions j < len whose slot is the
// row's own (a slot) or collapses onto the row's word (a word) -- a gather: 64 positions a round, the hits taken in order from the ballot.
// `row0`: the call's row of this launch's row 0 (the host chunks the rows; the source row is (row0 + row) / rows_per_src).
__global__ __launch_bounds__(256) void acg_score_finish_kernel(const float* __restrict__ pm, const float* __restrict__ ps, int nparts, int64_t rows,
                                                               int64_t row0, int64_t rows_per_src, const int* __restrict__ word,
                                                               const int* __restrict__ slot, const float* __restrict__ o, int K,
                                                               const float* __restrict__ copy_w, const float* __restrict__ copy_b,
                                                               const float* __restrict__ attn, int64_t attn_stride, const int64_t* __restrict__ lens,
                                                               int QL, const int64_t* __restrict__ map, const int64_t* __restrict__ e2t, int CV,
                                                               float* __restrict__ token_logp) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                                  // wave-uniform
    const int w = word[row], sl = slot[row];
    if (sl == ACG_SCORE_MASKED) {
        if (lane == 0) token_logp[row] = 0.f;
        return;
    }
    // 1. the generator's statistics
    float gen = 0.f;                                                          // (1 - z) exp(l[w] - m) / Z, formed below
    float M = 0.f, S = 1.f;
    if (w >= 0) {
        float m = -INFINITY, s = 0.f;
        for (int p = lane; p < nparts; p += 64) {
            const int64_t at = (int64_t)p * rows + row;
            const float om = pm[at], os = ps[at];
            const float nm = fmaxf(m, om);
            if (nm > -INFINITY) s = s * expf(m - nm) + os * expf(om - nm);
            m = nm;
        }
        M = wave_max(m);
        S = wave_sum(m > -INFINITY ? s * expf(m - M) : 0.f);
    }
    // 2. the copy switch
    const float* ob = o + row * K;
    float x = 0.f;
    for (int k = 4 * lane; k < K; k += 256) {
        const float4 a = *reinterpret_cast<const float4*>(ob + k), cw = *reinterpret_cast<const float4*>(copy_w + k);
        x += (a.x * cw.x + a.y * cw.y) + (a.z * cw.z + a.w * cw.w);
    }
    x = wave_sum(x) + copy_b[0];
    const float z = 1.0f / (1.0f + expf(-x)), omz = 1.0f / (1.0f + expf(x));
    if (w >= 0) gen = omz * expf(token_logp[row] - M) / S;
    // 3. the copy mass of the row's word or slot
    const int64_t b = (row0 + row) / rows_per_src;
    const int64_t len64 = lens[b];                                            // clamped as int64: a length past 2^32 is QL, not its low word
    const int len = (int)(len64 < 0 ? 0 : (len64 > QL ? QL : len64));
    const int64_t* mb = map + b * QL;
    const int64_t* tb = e2t + b * CV;
    const float* ab = attn + row * attn_stride;
    float mass = 0.f;
    for (int j0 = 0; j0 < len; j0 += 64) {                                    // wave-uniform
        const int j = j0 + lane;
        float a = 0.f;
        bool hit = false;
        if (j < len) {
            const int64_t c = mb[j];
            if (c >= 0 && c < CV) {
                hit = w >= 0 ? (c >= 2 && tb[c] == (int64_t)w) : c == (int64_t)sl;
                if (hit) a = ab[j];
            }
        }
        unsigned long long hits = __ballot(hit);
        while (hits) {                                                        // ascending j, every lane the same sum
            const int src = __ffsll((long long)hits) - 1;
            mass += z * __shfl(a, src);
            hits &= hits - 1;
        }
    }
    // 4. log P
    if (lane == 0) token_logp[row] = logf(w >= 0 ? gen + mass : mass);
}

static size_t acg_score_ids_bytes(int64_t rows) { return 2 * align_up((size_t)rows * sizeof(int), 256); }

// one chunk of at most SCORE_ROW_CHUNK rows of the fused form; the pointers are the chunk's own, row0 its first row in the call
static int launch_acg_score_chunk(const float* o, const void* frag, const float* bias, int64_t VT, int64_t rows, int64_t row0, int64_t rows_per_src, int K,
                                  const int* word, const int* slot, const float* copy_w, const float* copy_b, const float* attn, int64_t attn_stride,
                                  const int64_t* lens, int QL, const int64_t* map, const int64_t* e2t, int CV, float* pm, float* ps, float* token_logp,
                                  hipStream_t st) {
    const int nvr = score_nvr(score_nrb(rows, K), (VT + 15) / 16), nparts = 4 * nvr;
    launch_score_gen_walk<true, int>("score_gen_target_kernel<pad>", o, frag, bias, VT, rows, K, nvr, word, token_logp, pm, ps, st);
    NIR_CHECK_LAUNCH("score_gen_target_kernel<pad>");
    {
        ProfScope ps_("acg_score_finish_kernel", st);
        hipLaunchKernelGGL(acg_score_finish_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, pm, ps, nparts, rows, row0, rows_per_src, word, slot, o,
                           K, copy_w, copy_b, attn, attn_stride, lens, QL, map, e2t, CV, token_logp);
    }
    NIR_CHECK_LAUNCH("acg_score_finish_kernel");
    return 0;
}

static bool acg_score_dims_ok(int64_t rows, int K, int64_t VT) {
    return rows >= 0 && rows < 0x7FFFFFFFLL && K >= 4 && K <= 8192 && K % 4 == 0 && VT > 0 && VT < 0x7FFFFFF0LL - ACG_MAX_CV;
}

}  // namespace nir

extern "C" size_t nir_score_gen_target_workspace_bytes(int64_t rows, int K, int64_t VT, int fused) {
    using namespace nir;
    if (rows <= 0 || rows >= 0x7FFFFFFFLL || K < 4 || K > 8192 || K % 4 || VT <= 0 || VT >= 0x7FFFFFF0LL) return 0;
    // fused: a fragment will be given -- the size of the form the entry then runs
    return fused && gen_fusable(K, VT) && !tun(g_tun.exact_f32) ? score_fused_bytes(rows, K, VT) : score_plain_bytes(rows, VT);
}

extern "C" int nir_score_gen_target(const float* x, int64_t rows, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                                    const int64_t* target, int64_t pad, void* workspace, size_t workspace_bytes, float* token_logp, float* lse,
                                    int32_t* id_flag, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(x && gen_w && target && token_logp, "score_gen_target: null pointer");
    NIR_REQUIRE(rows >= 0 && rows < 0x7FFFFFFFLL, "score_gen_target: rows outside [0, 2^31)");
    NIR_REQUIRE(K >= 4 && K <= 8192 && K % 4 == 0, "score_gen_target: K outside [4, 8192] or no multiple of 4");
    NIR_REQUIRE(VT > 0 && VT < 0x7FFFFFF0LL, "score_gen_target: VT outside [1, 2^31 - 16)");
    if (rows == 0) return 0;
    const bool fused = gen_frag != nullptr && gen_fusable(K, VT) && !tun(g_tun.exact_f32);
    if (!workspace || workspace_bytes < nir_score_gen_target_workspace_bytes(rows, K, VT, fused)) {
        set_error("score_gen_target: workspace null or too small");
        return NIR_ERR_WORKSPACE;
    }
    if (fused) {
        for (int64_t r0 = 0; r0 < rows; r0 += SCORE_ROW_CHUNK) {
            const int64_t n = std::min(SCORE_ROW_CHUNK, rows - r0);
            NIR_PROPAGATE(launch_score_gen_target(x + r0 * K, gen_frag, gen_b, VT, n, K, target + r0, pad, workspace, workspace_bytes, token_logp + r0,
                                                  lse ? lse + r0 : nullptr, id_flag, st));
        }
        return 0;
    }
    Workspace a(workspace, workspace_bytes);
    const int64_t ch = std::min(rows, score_plain_rows(VT));
    float* logits = a.take<float>((size_t)ch * VT);
    for (int64_t r0 = 0; r0 < rows; r0 += ch) {
        const int64_t n = std::min(ch, rows - r0);
        NIR_PROPAGATE(launch_linear(x + r0 * K, K, nullptr, nullptr, 0, 0, 0, gen_w, K, gen_b, nullptr, logits, VT, n, (int)VT, K, NIR_ACT_NONE, st));
        {
            ProfScope ps_("score_row_kernel", st);
            hipLaunchKernelGGL(score_row_kernel, dim3((unsigned)n), dim3(256), 0, st, logits, VT, target + r0, pad, token_logp + r0, lse ? lse + r0 : nullptr,
                               id_flag);
        }
        NIR_CHECK_LAUNCH("score_row_kernel");
    }
    return 0;
}

extern "C" int nir_score_sequences(float* token_logp, const int64_t* target, int64_t nseq, int T, int64_t pad, int64_t eos, float* scores, int64_t* lengths,
                                   nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(token_logp && target && scores && lengths, "score_sequences: null pointer");
    NIR_REQUIRE(nseq >= 0 && nseq < 0x7FFFFFFFLL && T > 0 && T <= (1 << 20), "score_sequences: bad dims");
    if (nseq == 0) return 0;
    {
        ProfScope ps_("score_sequences_kernel", (hipStream_t)stream);
        hipLaunchKernelGGL(score_sequences_kernel, g1(nseq), dim3(256), 0, (hipStream_t)stream, token_logp, target, nseq, T, pad, eos, scores, lengths);
    }
    NIR_CHECK_LAUNCH("score_sequences_kernel");
    return 0;
}

// ---- the copy generator's scorer (include/neuroir_acg_score.h) ---------------------------------------------------------------------------------------
extern "C" size_t nir_acg_score_gen_target_workspace_bytes(int64_t rows, int K, int64_t VT, int fused) {
    using namespace nir;
    if (rows <= 0 || !acg_score_dims_ok(rows, K, VT)) return 0;
    // the two int32 id arrays of the whole call, then the form's buffers: the partials of the largest chunk | the logits and one partial per row
    if (fused && gen_fusable(K, VT) && !tun(g_tun.exact_f32)) return acg_score_ids_bytes(rows) + score_fused_bytes(rows, K, VT);
    return acg_score_ids_bytes(rows) + score_plain_bytes(rows, VT) + 2 * align_up((size_t)std::min(rows, score_plain_rows(VT)) * sizeof(float), 256);
}

extern "C" int nir_acg_score_gen_target(const float* o, int64_t rows, int64_t rows_per_src, int K, const float* gen_w, const float* gen_b,
                                        const void* gen_frag, int64_t VT, const float* copy_w, const float* copy_b, const float* copy_attn,
                                        int64_t attn_stride, const int64_t* source_len, int QL, const int64_t* src_map_idx, const int64_t* ext2tgt, int CV,
                                        const int64_t* target, int64_t pad, void* workspace, size_t workspace_bytes, float* token_logp, int32_t* id_flag,
                                        nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(o && gen_w && copy_w && copy_b && copy_attn && source_len && src_map_idx && ext2tgt && target && token_logp,
                "acg_score_gen_target: null pointer");
    NIR_REQUIRE(rows >= 0 && rows < 0x7FFFFFFFLL, "acg_score_gen_target: rows outside [0, 2^31)");
    NIR_REQUIRE(K >= 4 && K <= 8192 && K % 4 == 0, "acg_score_gen_target: K outside [4, 8192] or no multiple of 4");
    NIR_REQUIRE(VT > 0 && VT < 0x7FFFFFF0LL - ACG_MAX_CV, "acg_score_gen_target: VT outside [1, 2^31 - 16 - %d)", ACG_MAX_CV);
    NIR_REQUIRE(acg_dims_ok(QL, CV), "acg_score_gen_target: QL outside [1, 4096] or CV outside [2, %d]", ACG_MAX_CV);
    NIR_REQUIRE(attn_stride >= QL, "acg_score_gen_target: attn_stride below QL");
    NIR_REQUIRE(rows_per_src >= 1 && rows % rows_per_src == 0, "acg_score_gen_target: rows_per_src must be at least 1 and divide rows");
    if (rows == 0) return 0;
    const bool fused = gen_frag != nullptr && gen_fusable(K, VT) && !tun(g_tun.exact_f32);
    if (!workspace || workspace_bytes < nir_acg_score_gen_target_workspace_bytes(rows, K, VT, fused)) {
        set_error("acg_score_gen_target: workspace null or too small");
        return NIR_ERR_WORKSPACE;
    }
    Workspace a(workspace, workspace_bytes);
    int* word = a.take<int>((size_t)rows);
    int* slot = a.take<int>((size_t)rows);
    {
        ProfScope ps_("acg_score_resolve_kernel", st);
        hipLaunchKernelGGL(acg_score_resolve_kernel, g1(rows), dim3(256), 0, st, target, rows, rows_per_src, VT, CV, ext2tgt, pad, word, slot, id_flag);
    }
    NIR_CHECK_LAUNCH("acg_score_resolve_kernel");
    if (fused) {
        const size_t ids = acg_score_ids_bytes(rows);
        for (int64_t r0 = 0; r0 < rows; r0 += SCORE_ROW_CHUNK) {
            const int64_t n = std::min(SCORE_ROW_CHUNK, rows - r0);
            Workspace c((char*)workspace + ids, workspace_bytes - ids);          // every chunk reuses the partials' room (one stream: in order)
            const size_t np = (size_t)score_nparts(n, K, VT) * n;
            float* pm = c.take<float>(np);
            float* ps = c.take<float>(np);
            NIR_PROPAGATE(launch_acg_score_chunk(o + r0 * K, gen_frag, gen_b, VT, n, r0, rows_per_src, K, word + r0, slot + r0, copy_w, copy_b,
                                                 copy_attn + r0 * attn_stride, attn_stride, source_len, QL, src_map_idx, ext2tgt, CV, pm, ps, token_logp + r0,
                                                 st));
        }
        return 0;
    }
    const int64_t ch = std::min(rows, score_plain_rows(VT));
    float* logits = a.take<float>((size_t)ch * VT);
    float* pm = a.take<float>((size_t)ch);
    float* ps = a.take<float>((size_t)ch);
    for (int64_t r0 = 0; r0 < rows; r0 += ch) {
        const int64_t n = std::min(ch, rows - r0);
        NIR_PROPAGATE(launch_linear(o + r0 * K, K, nullptr, nullptr, 0, 0, 0, gen_w, K, gen_b, nullptr, logits, VT, n, (int)VT, K, NIR_ACT_NONE, st));
        {
            ProfScope ps_("acg_score_row_kernel", st);
            hipLaunchKernelGGL(acg_score_row_kernel, dim3((unsigned)n), dim3(256), 0, st, logits, VT, word + r0, token_logp + r0, pm, ps);
        }
        NIR_CHECK_LAUNCH("acg_score_row_kernel");
        {
            ProfScope ps_("acg_score_finish_kernel", st);
            hipLaunchKernelGGL(acg_score_finish_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, pm, ps, 1, n, r0, rows_per_src, word + r0, slot + r0,
                               o + r0 * K, K, copy_w, copy_b, copy_attn + r0 * attn_stride, attn_stride, source_len, QL, src_map_idx, ext2tgt, CV,
                               token_logp + r0);
        }
        NIR_CHECK_LAUNCH("acg_score_finish_kernel");
    }
    return 0;
}
