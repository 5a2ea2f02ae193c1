// Beam search for the Seq2seq recommenders (include/neuroir_beam.h).  The reference has the state helpers of a beam
// (decoders/state.py:16-31 beam_update, :65-69 repeat_beam_size_times) and no search; they fix the row layout row = k B + b and the shuffle
// new[k] = old[backptr[b, k]].  The decode is the S2sStepper of csrc/seq2seq.hip (s2s_gen.hpp) over R = B W decode rows and B source rows, with
// the beam's tail behind it.  Per step, for all R rows at once:
//   (h,c) = cell(emb(tok), (h,c)); attention over source row `row % B` (the banks are not repeated); o = linear_out([ctx ; h])    S2sStepper::step
//   per row: lse and the W largest of y = W_g o + b_g         beam_gen_topk_kernel (the logits never leave the chip), or GEMM + beam_row_topk_kernel
//   per source row: the W best of the <= W W live candidates cum + (y - lse) and the frozen ones (finished beams)            beam_select_kernel
//   state rows gathered by the back-pointers                                                                                beam_reorder_kernel
// and once behind the loop beam_backtrack_kernel walks the stored back-pointers.  The global top-W over (k, v) lies inside the per-row top-W of
// the raw logits, since lse is constant within a row.  Everything is enqueued on the caller's stream; no host synchronisation, no allocation,
// no float atomics, every reduction in a fixed order.
// Every search in this file is that loop, and each part of it exists once: one generator top-k kernel (its rows fp32 or already split:
// BeamRowsF32 / BeamRowsSplit), one wave drain (beam_wave_pop_best), one selection (beam_select_rounds), one backtrack walk
// (beam_backtrack_walk), one carve of the partials (BeamPartials) and one tail on the host (BeamTail: begin, gen, select, reorder, end).
// ACG's search (include/neuroir_acg_beam.h) has another tail: the PAD-substituting forms of the two top-k kernels,
// acg_beam_row_kernel (the W best of a row's collapsed extended distribution) and the selection over extended ids (acg_beam_select_kernel).
// The session models' searches (include/neuroir_session_beam.h) put the tail behind the CARS step and behind the decoders
// without attention.  HredQS's search (include/neuroir_hredqs_beam.h) is the latter's loop (plain_beam_decode) with
// hq_beam_begin_kernel in front (pairing, repeat, split) and, in its fast form, the generator top-k on the split state the folded step leaves.
// The generator top-k kernel restates the staging, the chunk clamp and the fragment walk of the two greedy kernels, s2s_gen_argmax_kernel
// (s2s_gen.hpp) and hq_gen_argmax_kernel (csrc/hredqs.hip), whose code and register allocation stay as they are: a change to one of those has
// to be made in the greedy kernels too.  (One shared body with a tail policy was built and measured: the top-k and the keyed form ran slower
// than these bodies, outside their spread -- DESIGN.md section 21.)
#include <type_traits>
#include "s2s_gen.hpp"
#include "gen_rows.hpp"
#include "beam_steps.hpp"

namespace nir {

constexpr int BEAM_NONE = 0x7FFFFFFF;                 // the index of an empty list slot

// ---- sorted top-W lists on registers ---------------------------------------------------------------------------------------------------
// (a, ai) in front of (b, bi): the larger value, the smaller index among equals
__device__ __forceinline__ bool beam_before(float a, int ai, float b, int bi) { return a > b || (a == b && ai < bi); }

// Insert (y, v) into the descending list tv / ti.  Fully unrolled compare-exchange on constant indices: the lists stay in registers.
// TOTAL = false: values arrive in ascending index order, a plain `>` keeps the first index in front.  TOTAL = true: any arrival order.
template <int WM, bool TOTAL>
__device__ __forceinline__ void beam_insert(float (&tv)[WM], int (&ti)[WM], float y, int v) {
#pragma unroll
    for (int j = WM - 1; j >= 0; --j) {
        const bool here = TOTAL ? beam_before(y, v, tv[j], ti[j]) : y > tv[j];
        bool above = false;
        if (j > 0) above = TOTAL ? beam_before(y, v, tv[j - 1], ti[j - 1]) : y > tv[j - 1];
        const float pv = j > 0 ? tv[j - 1] : 0.f;
        const int pi = j > 0 ? ti[j - 1] : 0;
        tv[j] = above ? pv : (here ? y : tv[j]);
        ti[j] = above ? pi : (here ? v : ti[j]);
    }
}
template <int WM>
__device__ __forceinline__ void beam_pop(float (&tv)[WM], int (&ti)[WM], bool pop) {
#pragma unroll
    for (int j = 0; j < WM; ++j) {
        const float nv = j + 1 < WM ? tv[j + 1 < WM ? j + 1 : j] : -INFINITY;
        const int ni = j + 1 < WM ? ti[j + 1 < WM ? j + 1 : j] : BEAM_NONE;
        tv[j] = pop ? nv : tv[j];
        ti[j] = pop ? ni : ti[j];
    }
}

template <int CTRL>
__device__ __forceinline__ int dpp_mov_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ int wave_min_i(int v) {
    v = min(v, dpp_mov_i<0xB1>(v));
    v = min(v, dpp_mov_i<0x4E>(v));
    v = min(v, dpp_mov_i<0x141>(v));
    v = min(v, dpp_mov_i<0x140>(v));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// One round of the drain that merges the sorted lists of a wave's 64 lanes: (mx, mi) is the largest head, the smallest index among equals, in
// every lane; its owner pops.  W rounds give the wave's W best in order.  (The loop stays with the caller: inside the helper it compiles to
// another schedule of the row kernels.)
template <int WM>
__device__ __forceinline__ void beam_wave_pop_best(float (&tv)[WM], int (&ti)[WM], float& mx, int& mi) {
    const float hv = tv[0];
    const int hi = ti[0];
    mx = wave_max(hv);
    mi = wave_min_i(hv == mx ? hi : BEAM_NONE);
    beam_pop<WM>(tv, ti, hv == mx && hi == mi);
}

// ---- generator + bias + (lse, top-W): logits[b, v] = x[b, :] . W[v, :] + bias[v] never leave the chip --------------------------------------
// The staging, tiling, fragment format and chunked prefetch of the greedy kernels (see the head of the file).  In the place of their (best,
// index) every lane keeps, per batch tile, the online-softmax pair (max, sum) and a sorted list of its WM largest biased logits with their
// indices: one threshold test per value, an insertion only when it passes.  The four lanes of a decode row are merged in the wave (WM rounds:
// the best of the four heads wins, its owner pops); every wave writes one partial per decode row -- pval / pidx [part][Bd][W], pm / ps
// [part][Bd] -- and beam_merge_row reduces the partials of all waves and workgroups.  The logit is the greedy kernels' expression: W = 1 picks
// their token.
// PAD (the copy generator's beam): the logit of v == 0 is replaced by ACG_PAD_LOGIT before the online-softmax pair and the
// list insert, as STATS does in s2s_gen_argmax_kernel.  PAD = false compiles to the kernel without the test.
// ROWSRC (gen_rows.hpp: BeamRowsF32, BeamRowsSplit): where the decode rows come from and how the grid maps to (row block, vocabulary range) --
// the only two things the forms differ in.  The kernel stages its NR = 16 NBT rows from b0 on into the LDS planes [2 terms][NR][K + 8] in K/4 chunks a row (zero rows past Bd; the loads
// of SB trips are issued, unconditionally and from a clamped row, before the first is written): load() reads chunk c of a row, store() puts it
// into the planes.  map() reads blockIdx of a grid of nvr ranges x ceil(Bd / NR) row blocks.  The mapping is a speed choice: any placement
// gives the same partials up to the order of the parts, which the merge's tie rule does not depend on.
template <class ROWSRC, int NBT, int WM, bool PAD>
__global__ __launch_bounds__(256, 1) void beam_gen_topk_kernel(const typename ROWSRC::elem* __restrict__ x, const _Float16* __restrict__ wfrag,
                                                               const float* __restrict__ bias, int64_t VT, int64_t ntiles, int64_t Bd, int K, int nvr,
                                                               int W, float* __restrict__ pval, int* __restrict__ pidx, float* __restrict__ pm,
                                                               float* __restrict__ ps) {
    extern __shared__ __attribute__((aligned(16))) _Float16 beam_sm[];         // [2 terms][ROWS][LD]
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
        const int K4 = K / 4, total = ROWS * K4;                                  // K/4 chunks a row in either form; total a multiple of 256
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
                    ROWSRC::template store<ROWS>(beam_sm, r, c, LD, v);
                }
            }
        }
    }
    __syncthreads();
    float tv[NBT][WM], rm[NBT], rs[NBT];
    int ti[NBT][WM];
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) {
        rm[bt] = -INFINITY;
        rs[bt] = 0.f;
#pragma unroll
        for (int j = 0; j < WM; ++j) { tv[bt][j] = -INFINITY; ti[bt][j] = BEAM_NONE; }
    }
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
    const _Float16* bp0 = beam_sm + c16 * LD + 8 * g4;
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
                    y[r] = fmaf(acx[bt][r], SPLIT2_INV, acc[bt][r]) + bv[r];  // the greedy kernel's expression: W = 1 picks its token
                    if constexpr (PAD) {
                        if (v0 + r == 0) y[r] = ACG_PAD_LOGIT;                // the reference assigns this constant behind the linear
                    }
                    if (v0 + r >= VT) y[r] = -INFINITY;                       // padded tile rows: never kept, add exp(-inf) = 0
                    m = fmaxf(m, y[r]);
                }
                if (m > -INFINITY) {
                    rs[bt] = rs[bt] * __expf(rm[bt] - m) + ((__expf(y[0] - m) + __expf(y[1] - m)) + (__expf(y[2] - m) + __expf(y[3] - m)));
                    rm[bt] = m;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)                                   // ascending in r: '>' keeps the first index in front
                    if (y[r] > tv[bt][WM - 1]) beam_insert<WM, false>(tv[bt], ti[bt], y[r], (int)(v0 + r));
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
    // lanes l, l + 16, l + 32, l + 48 hold the same decode row: the sums combine (under fp contraction the two lanes of a pair may differ in the
    // last bit; only the g4 == 0 lane's value is written), the lists merge head by head by comparisons alone
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
        const int64_t slot = ((int64_t)vr * 4 + wave) * Bd + b;
        const bool writer = g4 == 0 && b < Bd;
        if (writer) { pm[slot] = rm[bt]; ps[slot] = rs[bt]; }
#pragma unroll
        for (int j = 0; j < WM; ++j) {
            const float hv = tv[bt][0];
            const int hi = ti[bt][0];
            float wv = hv;
            int wi = hi;
#pragma unroll
            for (int sh = 16; sh <= 32; sh <<= 1) {
                const float ov = __shfl_xor(wv, sh);
                const int oi = __shfl_xor(wi, sh);
                if (beam_before(ov, oi, wv, wi)) { wv = ov; wi = oi; }
            }
            beam_pop<WM>(tv[bt], ti[bt], hv == wv && hi == wi);
            if (writer && j < W) { pval[slot * W + j] = wv; pidx[slot * W + j] = wi; }
        }
    }
}

// ---- partial lists of one row -> (lse, top-W), one wave ------------------------------------------------------------------------------------
// pval / pidx [part][rows][stride] (the first W of a list are read), pm / ps [part][rows] (ps NULL: every sum is 1, so a single part with
// pm = lse passes through bit for bit).  Lane l takes parts l, l + 64, ... in order; the wave's maxima and sums combine through wave_max /
// wave_sum (a fixed tree) and the lists through W rounds of beam_wave_pop_best.  Lane 0 writes out_val / out_idx [W] and *out_lse.
// beam_merge_row_ms leaves the pair (max, sum) to the caller, in every lane, in the place of lse = max + log(sum).
__device__ __forceinline__ void beam_merge_row_ms(const float* pval, const int* pidx, const float* pm, const float* ps, int nparts, int64_t rows,
                                                  int64_t row, int stride, int W, int lane, float* out_val, int* out_idx, float& M, float& S) {
    constexpr int WM = NIR_BEAM_MAX_W;
    float tv[WM];
    int ti[WM];
#pragma unroll
    for (int j = 0; j < WM; ++j) { tv[j] = -INFINITY; ti[j] = BEAM_NONE; }
    float m = -INFINITY, s = 0.f;
    for (int p = lane; p < nparts; p += 64) {
        const int64_t slot = (int64_t)p * rows + row;
        const float om = pm[slot], os = ps ? ps[slot] : 1.f;
        const float nm = fmaxf(m, om);
        if (nm > -INFINITY) s = s * expf(m - nm) + os * expf(om - nm);
        m = nm;
        for (int j = 0; j < W; ++j) {
            const float y = pval[slot * stride + j];
            const int v = pidx[slot * stride + j];
            if (beam_before(y, v, tv[WM - 1], ti[WM - 1])) beam_insert<WM, true>(tv, ti, y, v);
        }
    }
    M = wave_max(m);
    S = wave_sum(m > -INFINITY ? s * expf(m - M) : 0.f);
    for (int j = 0; j < W; ++j) {
        float mx;
        int mi;
        beam_wave_pop_best<WM>(tv, ti, mx, mi);
        if (lane == 0) { out_val[j] = mx; out_idx[j] = mi; }
    }
}
__device__ __forceinline__ void beam_merge_row(const float* pval, const int* pidx, const float* pm, const float* ps, int nparts, int64_t rows,
                                               int64_t row, int stride, int W, int lane, float* out_val, int* out_idx, float* out_lse) {
    float M, S;
    beam_merge_row_ms(pval, pidx, pm, ps, nparts, rows, row, stride, W, lane, out_val, out_idx, M, S);
    if (lane == 0) *out_lse = M + logf(S);
}

__global__ __launch_bounds__(64) void beam_topk_finish_kernel(const float* __restrict__ pval, const int* __restrict__ pidx, const float* __restrict__ pm,
                                                              const float* __restrict__ ps, int nparts, int64_t rows, int W,
                                                              float* __restrict__ top_val, int* __restrict__ top_idx, float* __restrict__ lse) {
    const int64_t row = blockIdx.x;
    beam_merge_row(pval, pidx, pm, ps, nparts, rows, row, W, W, threadIdx.x, top_val + row * W, top_idx + row * W, lse + row);
}

// ---- the HredQS beam's first state, one launch: pairing, repeat and split --------------------------------------------------------------------------
// hs / cs [B, S, H] (session b, step s at row b S + s) -> h0 / c0 [R = Bd W, H]: beam row k Bd + i takes the state of step i / B of session
// i % B (hq_pair_kernel's pairing, on SOURCE rows); h16 (optional): h0 as the fp16 term pairs of the folded step, [row][H/8][2][8], in
// hq_pair_kernel's expressions.
__global__ void hq_beam_begin_kernel(const float* __restrict__ hs, const float* __restrict__ cs, int64_t B, int64_t S, int H, int64_t n,
                                     float* __restrict__ h0, float* __restrict__ c0, _Float16* __restrict__ h16) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;                                                       // n = R H
    const int64_t r = e / H, i = r % (B * S);
    const int k = (int)(e - r * H);
    const int64_t src = ((i % B) * S + i / B) * H + k;
    const float v = hs[src];
    h0[e] = v;
    c0[e] = cs[src];
    if (h16) {
        const _Float16 a = split2_hi1_rne(v);
        _Float16* d = h16 + (e >> 3) * 16 + (e & 7);
        d[0] = a;
        d[8] = split2_lo1(v, a);
    }
}

// ---- plain form: one workgroup per row of [rows, VT] logits -> (lse, top-W), the same tie rule ---------------------------------------------
// PAD (the copy generator's beam): logits[row, 0] is read as ACG_PAD_LOGIT, and the row's pair comes out apart -- max in `lse`, sum in `psum` --
// the partial format acg_beam_row_kernel merges (one part per row).  PAD = false never touches psum.
template <bool PAD = false>
__global__ __launch_bounds__(256) void beam_row_topk_kernel(const float* __restrict__ logits, int64_t VT, int W, float* __restrict__ top_val,
                                                            int* __restrict__ top_idx, float* __restrict__ lse, float* __restrict__ psum) {
    constexpr int WM = NIR_BEAM_MAX_W;
    __shared__ float lv[256 * WM];
    __shared__ int li[256 * WM];
    __shared__ float lm[256], ls[256];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const float* y = logits + row * VT;
    float tv[WM];
    int ti[WM];
#pragma unroll
    for (int j = 0; j < WM; ++j) { tv[j] = -INFINITY; ti[j] = BEAM_NONE; }
    float m = -INFINITY, s = 0.f;
    for (int64_t v = tid; v < VT; v += 256) {                                 // ascending: '>' keeps the first index in front
        float a = y[v];
        if constexpr (PAD) {
            if (v == 0) a = ACG_PAD_LOGIT;
        }
        const float nm = fmaxf(m, a);
        if (nm > -INFINITY) s = s * expf(m - nm) + expf(a - nm);
        m = nm;
        if (a > tv[WM - 1]) beam_insert<WM, false>(tv, ti, a, (int)v);
    }
#pragma unroll
    for (int j = 0; j < WM; ++j) { lv[tid * WM + j] = tv[j]; li[tid * WM + j] = ti[j]; }
    lm[tid] = m;
    ls[tid] = s;
    __syncthreads();
    if constexpr (PAD) {
        if (tid < 64) {
            float M, S;
            beam_merge_row_ms(lv, li, lm, ls, 256, 1, 0, WM, W, tid, top_val + row * W, top_idx + row * W, M, S);
            if (tid == 0) { lse[row] = M; psum[row] = S; }
        }
    } else {
        if (tid < 64) beam_merge_row(lv, li, lm, ls, 256, 1, 0, WM, W, tid, top_val + row * W, top_idx + row * W, lse + row);
    }
}

// ---- selection: one wave per source row ----------------------------------------------------------------------------------------------------
// Per beam k of source row b (decode row k B + b): the partials merge to lse and the top-W logits; lane k W + j then holds candidate j of
// beam k -- live: cum[b, k] + (y - lse), token v; finished: j = 0 alone, (cum[b, k], EOS).  W rounds pick (score descending, k ascending, v
// ascending: the flat index k VT + v).  cum and finished are read before anything is written, so they update in place.
// beam_select_rounds is the selection of source row b by one wave, behind whatever produced the lists.  cand(k, j, y, v): the log-probability
// and the id of candidate j of the live beam k; ids outside [0, nid) read as 0; fed(tokv): the source-side id the next step reads for token
// tokv (<unk> outside [0, Vsrc)).
template <class Cand, class Fed>
__device__ __forceinline__ void beam_select_rounds(int64_t b, int64_t B, int W, int lane, int64_t nid, int64_t Vsrc, Cand cand, Fed fed,
                                                   float* __restrict__ cum, int* __restrict__ finished, int* __restrict__ backptr,
                                                   int* __restrict__ token, int64_t* __restrict__ next_ids) {
    const int k = lane / W, j = lane - k * W;
    bool open = false;                                                        // a candidate not yet taken
    float score = -INFINITY;
    int v = BEAM_NONE;
    if (k < W) {
        const float ck = cum[b * W + k];
        if (finished[b * W + k]) {
            open = j == 0;
            score = ck;
            v = NIR_BEAM_EOS;
        } else {
            float y;
            cand(k, j, y, v);
            open = true;
            score = ck + y;
        }
        if (!(score == score)) score = -INFINITY;                             // a NaN never wins and never stalls the rounds
    }
    for (int o = 0; o < W; ++o) {
        const float sc = open ? score : -INFINITY;
        const float mx = wave_max(sc);
        const bool c1 = open && sc == mx;
        const int mk = wave_min_i(c1 ? k : BEAM_NONE);
        const bool c2 = c1 && k == mk;
        const int mv = wave_min_i(c2 ? v : BEAM_NONE);
        if (c2 && v == mv) {
            open = false;
            const int64_t tokv = (v >= 0 && (int64_t)v < nid) ? v : 0;
            const int64_t slot = b * W + o;
            cum[slot] = score;
            finished[slot] = tokv == NIR_BEAM_EOS;                             // (a frozen candidate's token is EOS too)
            backptr[slot] = k;
            token[slot] = (int)tokv;
            const int64_t nxt = fed(tokv);
            next_ids[(int64_t)o * B + b] = (nxt >= 0 && nxt < Vsrc) ? nxt : 1;
        }
    }
}
__global__ __launch_bounds__(64) void beam_select_kernel(const float* __restrict__ pval, const int* __restrict__ pidx, const float* __restrict__ pm,
                                                         const float* __restrict__ ps, int nparts, int64_t B, int W, int64_t VT,
                                                         const int64_t* __restrict__ lut, int64_t Vsrc, float* __restrict__ cum,
                                                         int* __restrict__ finished, int* __restrict__ backptr, int* __restrict__ token,
                                                         int64_t* __restrict__ next_ids) {
    constexpr int WM = NIR_BEAM_MAX_W;
    __shared__ float cval[WM * WM], clse[WM];
    __shared__ int cidx[WM * WM];
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    for (int k = 0; k < W; ++k) {
        if (finished[b * W + k]) continue;                                    // wave-uniform: a finished beam's logits are not read
        beam_merge_row(pval, pidx, pm, ps, nparts, B * W, (int64_t)k * B + b, W, W, lane, cval + k * W, cidx + k * W, clse + k);
    }
    __syncthreads();
    beam_select_rounds(
        b, B, W, lane, VT, Vsrc,
        [&](int k, int j, float& y, int& v) {
            y = cval[k * W + j] - clse[k];
            v = cidx[k * W + j];
        },
        [&](int64_t tokv) { return lut ? lut[tokv] : tokv; }, cum, finished, backptr, token, next_ids);
}

// ---- the copy generator's beam (include/neuroir_acg_beam.h) -------------------------------------------------------------
// One wave per beam row r = k nsrc + b: the W best (log P, extended id) of the row's COLLAPSED extended distribution, which is never written.
// Steps 1-3 are those of acg_select_kernel (csrc/acg.hip), in its fp32 expressions: the partials merge to (m, Z) and the raw top-W list (PAD
// already substituted by the producer), z = sigmoid(x) and 1 - z = sigmoid(-x), the copy mass of every slot (j ascending) and the slots' targets
// in LDS.  The maps, ext2tgt and the length are those of source row b; o and the copy attention are the beam row's own.  Candidates:
//   a slot that is not collapsed                     mass[c]                                             id VT + c
//   a raw top-W entry that no slot collapses onto    (1 - z) exp(l[v] - m) / Z                           id v
//   a target t of one or more slots                  (1 - z) exp(l[t] - m) / Z + the slots' mass, once   id t   (l[t]: the fp32 row dot)
// A collapsed slot is no candidate, and a raw entry that is a target is dropped for the third form.  Every lane keeps a sorted list of its
// offers (any arrival order: beam_insert<TOTAL>); W rounds of (largest head, smallest id among equals) merge them.  log 0 = -inf is a
// candidate like any other: it loses to every finite one and is ordered by id among its kind.  `finished` [nsrc, W] (optional): the rows of
// finished beams are skipped, their outputs left as they are -- the selection does not read them.
// LT (the sampler's plain top-k form, csrc/sample.hip): a target's logit is read from the GEMM's workspace `logits` [R, VT] -- what m and Z were
// formed from -- instead of the wave's row dot.  LT = false is the beam's kernel, to the instruction; `logits` is not read there.
template <bool LT = false>
__global__ __launch_bounds__(64) void acg_beam_row_kernel(const float* __restrict__ o, int K, const float* __restrict__ gen_w, const float* __restrict__ gen_b,
                                                          int64_t VT, const float* __restrict__ pval, const int* __restrict__ pidx,
                                                          const float* __restrict__ pm, const float* __restrict__ ps, int nparts, int64_t R, int64_t nsrc,
                                                          int W, const float* __restrict__ copy_w, const float* __restrict__ copy_b,
                                                          const float* __restrict__ attn, int64_t attn_stride, const int64_t* __restrict__ lens, int QL,
                                                          const int64_t* __restrict__ map, const int64_t* __restrict__ e2t, int CV,
                                                          const int* __restrict__ finished, float* __restrict__ top_val, int* __restrict__ top_idx,
                                                          const float* __restrict__ logits) {
    constexpr int WM = NIR_BEAM_MAX_W;
    extern __shared__ float acgb_sm[];                         // mass [CV] floats, tl [CV] ints
    __shared__ float rv[WM];
    __shared__ int ri[WM];
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x, b = r % nsrc;
    if (finished && finished[b * W + r / nsrc]) return;        // uniform over the workgroup (one wave)
    float* mass = acgb_sm;
    int* tl = reinterpret_cast<int*>(acgb_sm + CV);
    // 1. the generator's statistics and the raw top-W
    float m, Z;
    beam_merge_row_ms(pval, pidx, pm, ps, nparts, R, r, W, W, lane, rv, ri, m, Z);
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
    __syncthreads();                                           // (one wave: the LDS writes above, rv / ri among them, are visible below)
    // 4. the candidates
    float tv[WM];
    int ti[WM];
#pragma unroll
    for (int j = 0; j < WM; ++j) { tv[j] = -INFINITY; ti[j] = BEAM_NONE; }
    auto offer = [&](float P, int e) {
        const float lp = logf(P);
        if (beam_before(lp, e, tv[WM - 1], ti[WM - 1])) beam_insert<WM, true>(tv, ti, lp, e);
    };
    for (int c = lane; c < CV; c += 64)
        if (tl[c] < 0) offer(mass[c], (int)(VT + c));
    for (int j = 0; j < W; ++j) {                              // wave-uniform
        const int v = ri[j];
        if (v < 0 || v >= VT) continue;
        int hit = 0;
        for (int c = lane; c < CV; c += 64) hit |= tl[c] == v;
        if (__any(hit)) continue;
        if (lane == 0) offer(omz * expf(rv[j] - m) / Z, v);
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
        if constexpr (LT) {
            if (t != 0) lt = logits[r * VT + t];
        } else if (t != 0) {
            const float* wr = gen_w + (int64_t)t * K;
            float d = 0.f;
            for (int k = 4 * lane; k < K; k += 256) {
                const float4 a = *reinterpret_cast<const float4*>(ob + k), w = *reinterpret_cast<const float4*>(wr + k);
                d += (a.x * w.x + a.y * w.y) + (a.z * w.z + a.w * w.w);
            }
            lt = wave_sum(d) + (gen_b ? gen_b[t] : 0.f);
        }
        if (lane == 0) offer(omz * expf(lt - m) / Z + cp, t);
    }
    for (int j = 0; j < W; ++j) {
        float mx;
        int mi;
        beam_wave_pop_best<WM>(tv, ti, mx, mi);
        if (lane == 0) { top_val[r * W + j] = mx; top_idx[r * W + j] = mi; }
    }
}

// beam_select_rounds over finished per-row lists (top_val = log P, lse NULL = 0) of EXTENDED ids in [0, VT + CV): the flat index is
// k (VT + CV) + e, finished means e == EOS, and the token fed back is lut[e] below VT and e2s[b, e - VT] from VT on.
__global__ __launch_bounds__(64) void acg_beam_select_kernel(const float* __restrict__ top_val, const int* __restrict__ top_idx, const float* __restrict__ lse,
                                                             int64_t B, int W, int64_t VT, int CV, const int64_t* __restrict__ lut,
                                                             const int64_t* __restrict__ e2s, int64_t Vsrc, float* __restrict__ cum,
                                                             int* __restrict__ finished, int* __restrict__ backptr, int* __restrict__ token,
                                                             int64_t* __restrict__ next_ids) {
    const int64_t b = blockIdx.x;
    beam_select_rounds(
        b, B, W, threadIdx.x, VT + CV, Vsrc,
        [&](int k, int j, float& y, int& v) {
            const int64_t row = (int64_t)k * B + b;
            y = top_val[row * W + j] - (lse ? lse[row] : 0.f);
            v = top_idx[row * W + j];
        },
        [&](int64_t tokv) { return tokv < VT ? (lut ? lut[tokv] : tokv) : e2s[b * CV + (tokv - VT)]; }, cum, finished, backptr, token, next_ids);
}

__global__ void beam_init_kernel(float* __restrict__ cum, int* __restrict__ finished, int64_t n, int W) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    cum[e] = e % W == 0 ? 0.f : -INFINITY;
    finished[e] = 0;
}

// ---- the state shuffle: out row k B + b = in row backptr[b, k] B + b, for up to three states of H floats (4 H bytes) per row ------------------
__global__ __launch_bounds__(256) void beam_reorder_kernel(const int* __restrict__ backptr, int64_t B, int W, int H4, const float4* __restrict__ i0,
                                                           float4* __restrict__ o0, const float4* __restrict__ i1, float4* __restrict__ o1,
                                                           const float4* __restrict__ i2, float4* __restrict__ o2) {
    const int64_t r = blockIdx.x;                                             // k B + b
    const int64_t k = r / B, b = r - k * B;
    int src = backptr[b * W + k];
    src = src < 0 ? 0 : (src >= W ? W - 1 : src);
    const int64_t s = (int64_t)src * B + b;
    for (int f = threadIdx.x; f < H4; f += 256) {
        o0[r * H4 + f] = i0[s * H4 + f];
        if (i1) o1[r * H4 + f] = i1[s * H4 + f];
        if (i2) o2[r * H4 + f] = i2[s * H4 + f];
    }
}

// ---- backtrack: output beam j of source row b, walked from the last step through the back-pointers ---------------------------------------------
// tok / bp [max_len][B][W]; attn_ws [max_len][R][QL], the rows as the attention launch of each step wrote them (a step's row belongs to the
// beam the candidate extended: backptr).
// The walk of output o = b W + j: the token of every step into pred, the length up to the first EOS, the score; `writer`: this thread writes
// them.  step(t, b, src): called per step with the (clamped) beam the candidate extended.
template <class Step>
__device__ __forceinline__ void beam_backtrack_walk(const int* __restrict__ tok, const int* __restrict__ bp, const float* __restrict__ cum, int64_t B,
                                                    int W, int max_len, int64_t o, bool writer, int64_t* __restrict__ pred,
                                                    float* __restrict__ scores, int64_t* __restrict__ lengths, Step step) {
    const int64_t b = o / W;
    int k = (int)(o - b * W);
    int len = max_len;
    for (int t = max_len - 1; t >= 0; --t) {
        const int64_t slot = ((int64_t)t * B + b) * W + k;
        const int tk = tok[slot];
        int src = bp[slot];
        src = src < 0 ? 0 : (src >= W ? W - 1 : src);
        if (tk == NIR_BEAM_EOS) len = t + 1;
        if (writer) pred[o * max_len + t] = tk;
        step(t, b, src);
        k = src;
    }
    if (writer) { scores[o] = cum[o]; lengths[o] = len; }
}
// one wave per output: the lanes copy the attention rows
__global__ __launch_bounds__(64) void beam_backtrack_kernel(const int* __restrict__ tok, const int* __restrict__ bp, const float* __restrict__ attn_ws,
                                                            const float* __restrict__ cum, int64_t B, int W, int max_len, int QL,
                                                            int64_t* __restrict__ pred, float* __restrict__ scores, int64_t* __restrict__ lengths,
                                                            float* __restrict__ attn) {
    const int64_t o = blockIdx.x;
    const int lane = threadIdx.x;
    beam_backtrack_walk(tok, bp, cum, B, W, max_len, o, lane == 0, pred, scores, lengths, [&](int t, int64_t b, int src) {
        const float* ar = attn_ws + (((int64_t)t * W + src) * B + b) * QL;
        float* ao = attn + (o * max_len + t) * QL;
        for (int q = lane; q < QL; q += 64) ao[q] = ar[q];
    });
}
// without attention rows: one thread per output
__global__ __launch_bounds__(256) void beam_backtrack_tokens_kernel(const int* __restrict__ tok, const int* __restrict__ bp, const float* __restrict__ cum,
                                                                    int64_t B, int W, int max_len, int64_t* __restrict__ pred, float* __restrict__ scores,
                                                                    int64_t* __restrict__ lengths) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= B * W) return;
    beam_backtrack_walk(tok, bp, cum, B, W, max_len, o, true, pred, scores, lengths, [](int, int64_t, int) {});
}

// out row r = in row r % Bd for the two states (H4 float4 per row), and map_out[r] = map_in[r % Bd] (map_in NULL: no map): the first state of
// the session models' beams, whose callers repeat nothing
__global__ __launch_bounds__(256) void beam_repeat_kernel(const float4* __restrict__ h_in, const float4* __restrict__ c_in, int64_t Bd, int H4,
                                                          float4* __restrict__ h_out, float4* __restrict__ c_out, const int64_t* __restrict__ map_in,
                                                          int64_t* __restrict__ map_out) {
    const int64_t r = blockIdx.x, i = r % Bd;
    for (int f = threadIdx.x; f < H4; f += 256) {
        h_out[r * H4 + f] = h_in[i * H4 + f];
        c_out[r * H4 + f] = c_in[i * H4 + f];
    }
    if (map_in && threadIdx.x == 0) map_out[r] = map_in[i];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------------
// The partials of a top-k producer in a workspace: pval / pidx [parts][rows][W], pm / ps [parts][rows] (sums = false: a producer that writes no
// sums -- the row kernel's single part with pm = lse -- and ps NULL).  beam_partials_bytes: what these four takes and `takes` - 4 further ones
// around them need at most.
struct BeamPartials {
    float *pval, *pm, *ps;
    int* pidx;
    void take(Workspace& a, size_t parts, int64_t rows, int W, bool sums) {
        pval = a.take<float>(parts * rows * W);
        pidx = a.take<int>(parts * rows * W);
        pm = a.take<float>(parts * rows);
        ps = sums ? a.take<float>(parts * rows) : nullptr;
    }
};
static size_t beam_partials_bytes(size_t parts, int64_t rows, int W, int takes) { return parts * rows * ((size_t)W * 8 + 8) + (size_t)takes * 256; }

// The dispatch over (NBT, WM) of one form of the fused generator: nbt row tiles a workgroup (gen_nbt), lists of 4 or NIR_BEAM_MAX_W entries.
// An instantiation's LDS limit is raised once, in front of its first launch.  name: the label of the profile and of the launch check.
template <class ROWSRC, bool PAD>
static int beam_gen_launch(const char* name, int nvr, int nbt, int64_t grid, const typename ROWSRC::elem* x, const void* frag, const float* bias, int64_t VT,
                           int64_t rows, int K, int W, const BeamPartials& p, hipStream_t st) {
    auto go = [&](auto nbt_c, auto wm_c) {
        constexpr int NBT = decltype(nbt_c)::value, WM = decltype(wm_c)::value;
        static const hipError_t raised = hipFuncSetAttribute((const void*)beam_gen_topk_kernel<ROWSRC, NBT, WM, PAD>,
                                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds(NBT == 4 ? 512 : 1024));
        (void)raised;
        hipLaunchKernelGGL((beam_gen_topk_kernel<ROWSRC, NBT, WM, PAD>), dim3((unsigned)grid), dim3(256), gen_lds(K), st, x, (const _Float16*)frag, bias, VT,
                           (VT + 15) / 16, rows, K, nvr, W, p.pval, p.pidx, p.pm, p.ps);
    };
    {
        ProfScope ps_(prof_shape_name(name, (long long)rows, (long long)VT, K), st);
        const std::integral_constant<int, 2> i2;
        const std::integral_constant<int, 4> i4;
        const std::integral_constant<int, 8> i8;
        if (nbt == 4 && W <= 4) go(i4, i4);
        else if (nbt == 4) go(i4, i8);
        else if (W <= 4) go(i2, i4);
        else go(i2, i8);
    }
    NIR_CHECK_LAUNCH(name);
    return 0;
}
// partials per decode row of the fused generator (one per wave of every vocabulary range); no rows: no row block to size a range by
static int beam_nparts(int64_t rows, int K, int64_t VT) { return rows > 0 ? 4 * s2s_nvr(rows, K, (VT + 15) / 16) : 0; }
// the fused generator on fp32 rows: beam_nparts partials a row (pad: the PAD-substituting instantiations of the copy generator's beam)
static int launch_beam_gen_topk(const float* x, const void* frag, const float* bias, int64_t VT, int64_t rows, int K, int W, const BeamPartials& p,
                                hipStream_t st, bool pad = false) {
    const int nbt = gen_nbt(K), nvr = s2s_nvr(rows, K, (VT + 15) / 16);
    const int64_t rb = (rows + 16 * nbt - 1) / (16 * nbt);
    if (pad) return beam_gen_launch<BeamRowsF32, true>("beam_gen_topk_kernel", nvr, nbt, nvr * rb, x, frag, bias, VT, rows, K, W, p, st);
    return beam_gen_launch<BeamRowsF32, false>("beam_gen_topk_kernel", nvr, nbt, nvr * rb, x, frag, bias, VT, rows, K, W, p, st);
}
// partials per beam row of the split-state generator: one per wave of every vocabulary range of hq_nvr's grid
static int hq_beam_nparts(int64_t rows, int K, int64_t VT) {
    return rows > 0 ? 4 * hq_nvr((rows + 16 * gen_nbt(K) - 1) / (16 * gen_nbt(K)), (VT + 15) / 16) : 0;
}
// the fused generator on the split state: hq_beam_nparts partials a row
static int launch_hq_beam_gen_topk(const _Float16* h16, const void* frag, const float* bias, int64_t VT, int64_t rows, int K, int W, const BeamPartials& p,
                                   hipStream_t st) {
    const int nbt = gen_nbt(K);
    const int64_t nrb = (rows + 16 * nbt - 1) / (16 * nbt);
    const int nvr = hq_nvr(nrb, (VT + 15) / 16);
    return beam_gen_launch<BeamRowsSplit, false>("hq_beam_gen_topk_kernel", nvr, nbt, nvr * nrb, h16, frag, bias, VT, rows, K, W, p, st);
}
// psum given: the PAD form, (max, sum) apart in lse / psum
static int launch_beam_row_topk(const float* logits, int64_t VT, int64_t rows, int W, float* top_val, int* top_idx, float* lse, hipStream_t st,
                                float* psum = nullptr) {
    {
        ProfScope ps_("beam_row_topk_kernel", st);
        if (psum) hipLaunchKernelGGL(beam_row_topk_kernel<true>, dim3((unsigned)rows), dim3(256), 0, st, logits, VT, W, top_val, top_idx, lse, psum);
        else hipLaunchKernelGGL(beam_row_topk_kernel<false>, dim3((unsigned)rows), dim3(256), 0, st, logits, VT, W, top_val, top_idx, lse, psum);
    }
    NIR_CHECK_LAUNCH("beam_row_topk_kernel");
    return 0;
}
static int launch_beam_select(const float* pval, const int* pidx, const float* pm, const float* ps, int nparts, int64_t B, int W, int64_t VT,
                              const int64_t* lut, int64_t V, float* cum, int* finished, int* backptr, int* token, int64_t* next_ids, hipStream_t st) {
    {
        ProfScope ps_("beam_select_kernel", st);
        hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)B), dim3(64), 0, st, pval, pidx, pm, ps, nparts, B, W, VT, lut, V, cum, finished, backptr, token,
                           next_ids);
    }
    NIR_CHECK_LAUNCH("beam_select_kernel");
    return 0;
}
static int launch_beam_reorder(const int* backptr, int64_t B, int W, int H, const float* h_in, float* h_out, const float* c_in, float* c_out,
                               const void* h16_in, void* h16_out, hipStream_t st) {
    {
        ProfScope ps_("beam_reorder_kernel", st);
        hipLaunchKernelGGL(beam_reorder_kernel, dim3((unsigned)(B * W)), dim3(256), 0, st, backptr, B, W, H / 4, (const float4*)h_in, (float4*)h_out,
                           (const float4*)c_in, (float4*)c_out, (const float4*)h16_in, (float4*)h16_out);
    }
    NIR_CHECK_LAUNCH("beam_reorder_kernel");
    return 0;
}
static bool beam_dims_ok(int W, int64_t VT) { return W >= 1 && W <= NIR_BEAM_MAX_W && VT >= W; }

// ---- the copy generator's beam: the two per-row launches, and the selection ---------------------------------------------------------------------
// partials of the PAD-substituting generator top-k (fused: gen_frag given; plain: GEMM into `logits` + the row kernel, one part per row, its sum
// in ps) -> acg_beam_row_kernel.  ps is needed in both forms.
static int launch_acg_beam_gen_select(const float* o, int64_t R, int64_t nsrc, int K, const float* gen_w, const float* gen_b, const void* gen_frag,
                                      int64_t VT, int W, float* logits, const BeamPartials& p, const float* copy_w, const float* copy_b,
                                      const float* attn, int64_t attn_stride, const int64_t* lens, int QL, const int64_t* map, const int64_t* e2t, int CV,
                                      const int* finished, float* top_val, int* top_idx, hipStream_t st, bool logit_targets = false) {
    int nparts = 1;
    if (gen_frag) {
        nparts = beam_nparts(R, K, VT);
        NIR_PROPAGATE(launch_beam_gen_topk(o, gen_frag, gen_b, VT, R, K, W, p, st, true));
    } else {
        NIR_PROPAGATE(launch_linear(o, K, nullptr, nullptr, 0, 0, 0, gen_w, K, gen_b, nullptr, logits, VT, R, (int)VT, K, NIR_ACT_NONE, st));
        NIR_PROPAGATE(launch_beam_row_topk(logits, VT, R, W, p.pval, p.pidx, p.pm, st, p.ps));
    }
    {
        ProfScope ps_("acg_beam_row_kernel", st);
        if (logit_targets && !gen_frag)
            hipLaunchKernelGGL(acg_beam_row_kernel<true>, dim3((unsigned)R), dim3(64), (size_t)2 * CV * sizeof(float), st, o, K, gen_w, gen_b, VT, p.pval, p.pidx,
                               p.pm, p.ps, nparts, R, nsrc, W, copy_w, copy_b, attn, attn_stride, lens, QL, map, e2t, CV, finished, top_val, top_idx, logits);
        else
            hipLaunchKernelGGL(acg_beam_row_kernel<false>, dim3((unsigned)R), dim3(64), (size_t)2 * CV * sizeof(float), st, o, K, gen_w, gen_b, VT, p.pval, p.pidx,
                               p.pm, p.ps, nparts, R, nsrc, W, copy_w, copy_b, attn, attn_stride, lens, QL, map, e2t, CV, finished, top_val, top_idx,
                               (const float*)nullptr);
    }
    NIR_CHECK_LAUNCH("acg_beam_row_kernel");
    return 0;
}
static int launch_acg_beam_select(const float* top_val, const int* top_idx, const float* lse, int64_t B, int W, int64_t VT, int CV, const int64_t* lut,
                                  const int64_t* e2s, int64_t V, float* cum, int* finished, int* backptr, int* token, int64_t* next_ids, hipStream_t st) {
    {
        ProfScope ps_("acg_beam_select_kernel", st);
        hipLaunchKernelGGL(acg_beam_select_kernel, dim3((unsigned)B), dim3(64), 0, st, top_val, top_idx, lse, B, W, VT, CV, lut, e2s, V, cum, finished, backptr,
                           token, next_ids);
    }
    NIR_CHECK_LAUNCH("acg_beam_select_kernel");
    return 0;
}
static bool acg_beam_dims_ok(int QL, int CV, int64_t VT) { return acg_dims_ok(QL, CV) && VT + CV < 0x7FFFFFFFLL; }

// ---- the tail of every search, on the host ---------------------------------------------------------------------------------------------------
// The beam's own buffers, behind a decoder's step buffers in its workspace, and the launches on them.  B source rows with W beams each are the
// R = B W decode rows (row k B + b); a step reads state slot 0 (the reordered one) and writes slot 1.
struct BeamTail {
    int64_t B, R;
    int W, max_len, nparts;                           // nparts: partials a row of the top-k producer (1: the row kernel, which writes no sums)
    BeamPartials part;
    int64_t* tgt;                                     // [R] the source-side ids the next step reads
    float* cum;                                       // [B, W]
    int *fin, *bp, *tok;                              // [B, W]; [max_len][B][W] each -- bp is the caller's `backptr` where given

    // takes the partials, tgt, cum, fin, (bp,) tok, in this order; sums: the producer writes ps
    void carve(Workspace& a, int64_t B_, int W_, int max_len_, int nparts_, bool sums, int32_t* backptr) {
        B = B_, W = W_, max_len = max_len_, nparts = nparts_, R = B_ * W_;
        part.take(a, (size_t)nparts, R, W, sums);
        tgt = a.take<int64_t>((size_t)R);
        cum = a.take<float>((size_t)R);
        fin = a.take<int>((size_t)R);
        bp = backptr ? backptr : a.take<int>((size_t)max_len * R);
        tok = a.take<int>((size_t)max_len * R);
    }
    // of every source row the first beam alone is alive (tgt is the caller's to fill: a stepper does it with its own launch)
    int begin(hipStream_t st) const {
        hipLaunchKernelGGL(beam_init_kernel, g1(R), dim3(256), 0, st, cum, fin, R, W);
        NIR_CHECK_LAUNCH("beam_init_kernel");
        return 0;
    }
    // the partials of the generator over x [R, K]: the fused kernel, or the fp32 GEMM into logits + one workgroup per row
    int gen(bool fused, const float* x, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT, float* logits, hipStream_t st) const {
        if (fused) return launch_beam_gen_topk(x, gen_frag, gen_b, VT, R, K, W, part, st);
        NIR_PROPAGATE(launch_linear(x, K, nullptr, nullptr, 0, 0, 0, gen_w, K, gen_b, nullptr, logits, VT, R, (int)VT, K, NIR_ACT_NONE, st));
        return launch_beam_row_topk(logits, VT, R, W, part.pval, part.pidx, part.pm, st);
    }
    int select(int step, int64_t VT, const int64_t* tgt2src, int64_t V, hipStream_t st) const {
        return launch_beam_select(part.pval, part.pidx, part.pm, part.ps, nparts, B, W, VT, tgt2src, V, cum, fin, bp + (int64_t)step * R,
                                  tok + (int64_t)step * R, tgt, st);
    }
    // behind all steps but the last: the state shuffle from slot 1 into slot 0 (c / h16 NULL: no such state)
    int reorder(int step, int H, float* const* h, float* const* c, float* const* h16, hipStream_t st) const {
        if (step + 1 >= max_len) return 0;
        return launch_beam_reorder(bp + (int64_t)step * R, B, W, H, h[1], h[0], c ? c[1] : nullptr, c ? c[0] : nullptr, h16 ? h16[1] : nullptr,
                                   h16 ? h16[0] : nullptr, st);
    }
    // the backtrack; attn_ws [max_len][R][QL] given: with the attention rows of every step, one wave per output
    int end(int64_t* predictions, float* scores, int64_t* lengths, hipStream_t st, const float* attn_ws = nullptr, int QL = 0,
            float* attentions = nullptr) const {
        const char* name = attn_ws ? "beam_backtrack_kernel" : "beam_backtrack_tokens_kernel";
        {
            ProfScope ps_(name, st);
            if (attn_ws)
                hipLaunchKernelGGL(beam_backtrack_kernel, dim3((unsigned)R), dim3(64), 0, st, tok, bp, attn_ws, cum, B, W, max_len, QL, predictions, scores,
                                   lengths, attentions);
            else
                hipLaunchKernelGGL(beam_backtrack_tokens_kernel, g1(R), dim3(256), 0, st, tok, bp, cum, B, W, max_len, predictions, scores, lengths);
        }
        NIR_CHECK_LAUNCH(name);
        return 0;
    }
};

struct BeamPlan {
    S2sStepBufs s;                                    // the stepper's buffers, over R = B W decode rows
    BeamTail t;
    float* attn;                                      // [max_len][R][QL] the attention rows of every step
    float* tval;                                      // ACG only: the rows' lists; a copy attention of its own
    int* tidx;
    AcgCopyAttn ca;
    size_t bytes;
};
// acg: 0 = Seq2seq, 1 = ACG with reuse_copy_attn, 2 = ACG with a copy attention of its own (its buffers lie behind everything Seq2seq's plan holds)
static BeamPlan beam_plan(void* ws, size_t cap, int64_t B, int QL, int W, int max_len, int H, int64_t VT, int attn_type, bool fused, int cell,
                          bool step16, int32_t* backptr, int acg = 0) {
    Workspace a(ws, cap);
    BeamPlan p;
    const int64_t R = B * W;
    p.s = s2s_step_bufs(a, R, B, QL, H, VT, attn_type, fused, cell, step16);               // (the fp16 term pairs with the fp16-term step only)
    p.t.carve(a, B, W, max_len, fused ? beam_nparts(R, H, VT) : 1, fused, backptr);
    p.s.tgt = p.t.tgt;
    p.attn = a.take<float>((size_t)max_len * R * QL);
    if (cell == S2S_CELL_GRU) p.s.gru = a.take<float>(gru_step_scratch_floats(R, H));
    p.tval = nullptr;
    p.tidx = nullptr;
    if (acg) {
        if (!fused) p.t.part.ps = a.take<float>((size_t)R);                                // the plain row kernel's sums
        p.tval = a.take<float>((size_t)R * W);
        p.tidx = a.take<int>((size_t)R * W);
    }
    if (acg == 2) p.ca.carve(a, R, B, QL, H, attn_type);
    p.bytes = align_up(a.off, 256);
    return p;
}
static size_t beam_decode_workspace_bytes(int64_t B, int QL, int W, int max_len, const nir_seq2seq_decoder_weights* w, int cell,
                                          const AcgDecode* acg = nullptr) {
    if (!s2s_weights_ok(w) || B < 0 || QL <= 0 || max_len <= 0 || !beam_dims_ok(W, w->VT)) return 0;
    if (acg && (!acg_weights_ok(w, acg) || !acg_beam_dims_ok(QL, acg->CV, w->VT))) return 0;
    return beam_plan(nullptr, 0, B, QL, W, max_len, w->H, w->VT, w->attn_type, s2s_fused(w), cell, s2s_step16(w), nullptr,
                     acg ? (acg->cw->reuse_copy_attn ? 1 : 2) : 0).bytes;
}

// The stepper of s2s_gen.hpp over W decode rows per source row, with the beam's tail behind the attentional output: top-k, select, reorder.  A
// step always reads state slot 0 (the reordered one) and writes slot 1; the attention rows of every step are kept for the backtrack.
static int s2s_beam_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, int W,
                           const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w,
                           void* workspace, size_t workspace_bytes, int64_t* predictions, float* scores, int64_t* lengths, float* attentions,
                           int32_t* backptr, int cell, hipStream_t st, const AcgDecode* acg = nullptr) {
    const int64_t R = B * W;
    S2sStepper s{acg ? "acg_beam_decode" : "beam_seq2seq_decode", w, cell, table, memory_bank, source_len, V, R, B, E, QL, st};
    NIR_PROPAGATE(s.check(dec_h, dec_c, predictions && scores && lengths && attentions, bos, max_len));
    NIR_REQUIRE(beam_dims_ok(W, w->VT), "beam_seq2seq_decode: beam width outside [1, %d] or above the target vocabulary", NIR_BEAM_MAX_W);
    NIR_REQUIRE(R < 0x7FFFFFFFLL, "beam_seq2seq_decode: too many decode rows");
    if (acg) {
        NIR_REQUIRE(acg_weights_ok(w, acg), "acg_beam_decode: copy weights incomplete for the attention type");
        NIR_REQUIRE(acg->src_map_idx && acg->ext2tgt && acg->ext2src, "acg_beam_decode: null index tensor");
        NIR_REQUIRE(acg_beam_dims_ok(QL, acg->CV, w->VT), "acg_beam_decode: CV outside [2, %d], or VT + CV too large", ACG_MAX_CV);
    }
    const int H = w->H;
    const bool fused = s.fused, step16 = s.step16, gru = cell == S2S_CELL_GRU;
    const BeamPlan p = beam_plan(workspace, workspace_bytes, B, QL, W, max_len, H, w->VT, w->attn_type, fused, cell, step16, backptr,
                                 acg ? (acg->cw->reuse_copy_attn ? 1 : 2) : 0);
    if (!workspace || p.bytes > workspace_bytes) {
        set_error("beam_seq2seq_decode: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
        return NIR_ERR_WORKSPACE;
    }
    if (B == 0) return 0;
    const BeamTail& t = p.t;
    s.b = p.s;
    NIR_PROPAGATE(s.prepare(dec_h, bos, p.s.h16[0]));
    NIR_PROPAGATE(t.begin(st));
    const float* hp = dec_h;
    const float* cp = dec_c;
    if (acg) NIR_PROPAGATE(p.ca.prepare(acg->cw, memory_bank, B, QL, H, w->attn_type, st));
    for (int step = 0; step < max_len; ++step) {
        NIR_PROPAGATE(s.step(hp, cp, p.s.h[1], p.s.c[1], p.s.h16[0], p.s.h16[1], p.attn + (int64_t)step * R * QL, QL));
        if (acg) {
            // ACG's tail: (a second attention whose query is the attentional output,) the W best of every row's collapsed extended distribution,
            // the selection over the source row's W W candidates
            const float* ca = p.attn + (int64_t)step * R * QL;
            int64_t ca_stride = QL;
            NIR_PROPAGATE(p.ca.step(acg->cw, p.s.ah, R, B, memory_bank, source_len, QL, H, w->attn_type, &ca, &ca_stride, st));
            NIR_PROPAGATE(launch_acg_beam_gen_select(p.s.ah, R, B, H, w->gen_w, w->gen_b, fused ? w->gen_frag : nullptr, w->VT, W, p.s.logits, t.part,
                                                     acg->cw->copy_w, acg->cw->copy_b, ca, ca_stride, source_len, QL, acg->src_map_idx, acg->ext2tgt, acg->CV, t.fin,
                                                     p.tval, p.tidx, st));
            NIR_PROPAGATE(launch_acg_beam_select(p.tval, p.tidx, nullptr, B, W, w->VT, acg->CV, tgt2src, acg->ext2src, V, t.cum, t.fin, t.bp + (int64_t)step * R,
                                                 t.tok + (int64_t)step * R, t.tgt, st));
        } else {
            NIR_PROPAGATE(t.gen(fused, p.s.ah, H, w->gen_w, w->gen_b, w->gen_frag, w->VT, p.s.logits, st));
            NIR_PROPAGATE(t.select(step, w->VT, tgt2src, V, st));
        }
        NIR_PROPAGATE(t.reorder(step, H, p.s.h, gru ? nullptr : p.s.c, step16 ? p.s.h16 : nullptr, st));
        hp = p.s.h[0];
        cp = p.s.c[0];
    }
    return t.end(predictions, scores, lengths, st, p.attn, QL, attentions);
}


// =================================================================================================================================================
// The session models' beams (include/neuroir_session_beam.h): the CARS decoder (csrc/cars_decode.hip's step over R = Bd W
// rows) and the decoders without attention of M_MATCH_TENSOR / MNSRF, with the tail above behind them.  "Source row" = decode row of the greedy
// decode: beam row r = k Bd + i reads what decode row i reads (memory bank rowmap[i], session term i).  Nothing is repeated by the caller.
// =================================================================================================================================================

// the first state of every beam row (and the repeated row map) into slot 0; h16first given: and its fp16 term pairs, for the fp16-term step
int launch_beam_repeat(const float* dec_h, const float* dec_c, int64_t Bd, int64_t R, int H, float* h0, float* c0, float* h16first,
                              const int64_t* map_in, int64_t* map_out, hipStream_t st) {
    hipLaunchKernelGGL(beam_repeat_kernel, dim3((unsigned)R), dim3(256), 0, st, (const float4*)dec_h, (const float4*)dec_c, Bd, H / 4, (float4*)h0, (float4*)c0,
                       map_in, map_out);
    NIR_CHECK_LAUNCH("beam_repeat_kernel");
    if (h16first) NIR_PROPAGATE(launch_h16_pack(h0, R * H, reinterpret_cast<_Float16*>(h16first), st));
    return 0;
}
// HredQS: pairing, repeat and split in one launch (hq_beam_begin_kernel) -- h0 / c0 [R, H] and, h16 given, the term pairs of h0
int launch_hq_beam_begin(const float* hs, const float* cs, int64_t B, int64_t S, int H, int64_t R, float* h0, float* c0, _Float16* h16, hipStream_t st) {
    hipLaunchKernelGGL(hq_beam_begin_kernel, g1(R * H), dim3(256), 0, st, hs, cs, B, S, H, R * H, h0, c0, h16);
    NIR_CHECK_LAUNCH("hq_beam_begin_kernel");
    return 0;
}
// ---- CARS ----------------------------------------------------------------------------------------------------------------------------------
// CarsRowsStep (beam_steps.hpp) over R = Bd W rows, every step from state slot 0 (the reordered one) into slot 1, with the tail above on p1.
struct CarsBeamPlan {
    CarsRowsStep s;
    float* logits;                                    // the plain generator's
    BeamTail t;
    size_t bytes;
};
static CarsBeamPlan cars_beam_plan(void* ws, size_t cap, int64_t rows_src, int64_t Bd, int QL, int W, int max_len, const nir_cars_decoder_weights* w,
                                   bool fused, int32_t* backptr) {
    Workspace a(ws, cap);
    CarsBeamPlan p;
    const int64_t R = Bd * W;
    p.s.carve(a, rows_src, R, QL, w);
    p.logits = a.take<float>(fused ? 0 : (size_t)R * w->VT);
    p.t.carve(a, Bd, W, max_len, fused ? beam_nparts(R, w->P, w->VT) : 1, fused, backptr);
    p.bytes = align_up(a.off, 256);
    return p;
}

}  // namespace nir

extern "C" size_t nir_beam_cars_decode_workspace_bytes(int64_t rows_src, int64_t Bd, int QL, int W, int max_len, const nir_cars_decoder_weights* w, int fused) {
    using namespace nir;
    if (!cars_beam_weights_ok(w) || rows_src < 0 || Bd < 0 || QL <= 0 || max_len <= 0 || !beam_dims_ok(W, w->VT)) return 0;
    return cars_beam_plan(nullptr, 0, rows_src, Bd, QL, W, max_len, w, fused && gen_fusable(w->P, w->VT) && !tun(g_tun.exact_f32), nullptr).bytes;
}

extern "C" int nir_beam_cars_decode(const float* dec_h, const float* dec_c, const float* encoded_source, const int64_t* source_len, int64_t rows_src, int QL,
                                    const int64_t* rowmap, int64_t Bd, const float* session_cat, const float* table, int64_t V, int E,
                                    const int64_t* tgt2src, int64_t bos, int max_len, const nir_cars_decoder_weights* w, const void* gen_frag, int W,
                                    void* workspace, size_t workspace_bytes, int64_t* predictions, float* scores, int64_t* lengths, int32_t* backptr,
                                    nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(dec_h && dec_c && encoded_source && source_len && rowmap && table && w && predictions && scores && lengths, "beam_cars_decode: null pointer");
    NIR_REQUIRE(cars_beam_weights_ok(w), "beam_cars_decode: null weight pointer or bad dims (HD, DQ, P multiples of 4)");
    NIR_REQUIRE(rows_src > 0 && Bd >= 0 && QL > 0 && max_len > 0 && V > 0 && E > 0 && E % 4 == 0, "beam_cars_decode: bad dims");
    NIR_REQUIRE(w->KS == 0 || (session_cat && w->sess_w), "beam_cars_decode: session representation / packed projector missing");
    NIR_REQUIRE(bos >= 0 && bos < V, "beam_cars_decode: BOS id outside the vocabulary");
    NIR_REQUIRE(beam_dims_ok(W, w->VT), "beam_cars_decode: beam width outside [1, %d] or above the target vocabulary", NIR_BEAM_MAX_W);
    NIR_REQUIRE(Bd * NIR_BEAM_MAX_W < 0x7FFFFFFFLL && w->VT < 0x7FFFFFF0LL, "beam_cars_decode: too many decode rows or target tokens");
    const int HD = w->HD, P = w->P;
    const int64_t R = Bd * W, VT = w->VT;
    const bool fused = s2s_gen_fused(gen_frag, P, VT);
    CarsBeamPlan p = cars_beam_plan(workspace, workspace_bytes, rows_src, Bd, QL, W, max_len, w, fused, backptr);
    const BeamTail& t = p.t;
    if (!workspace || p.bytes > workspace_bytes) {
        set_error("beam_cars_decode: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
        return NIR_ERR_WORKSPACE;
    }
    if (Bd == 0) return 0;
    NIR_PROPAGATE(p.s.prepare(dec_h, dec_c, encoded_source, source_len, rows_src, rowmap, Bd, session_cat, table, t.tgt, E, 0, st, [&] {
        const int rc = launch_fill_i64(t.tgt, bos, R, st);
        return rc != 0 ? rc : t.begin(st);
    }));
    for (int step = 0; step < max_len; ++step) {
        NIR_PROPAGATE(p.s.step(0, 1));
        NIR_PROPAGATE(t.gen(fused, p.s.p1, P, w->pred2_w, nullptr, gen_frag, VT, p.logits, st));
        NIR_PROPAGATE(t.select(step, VT, tgt2src, V, st));
        NIR_PROPAGATE(t.reorder(step, HD, p.s.h, p.s.c, p.s.step16 ? p.s.h16 : nullptr, st));
    }
    return t.end(predictions, scores, lengths, st);
}

// ---- the decoders without attention (M_MATCH_TENSOR, MNSRF): nir_decode_greedy_plain_folded's step over R rows ------------------------------------
namespace nir {
struct PlainBeamPlan {
    float *h[2], *c[2], *h16[2], *logits;             // (logits: the plain generator's)
    BeamTail t;
    size_t bytes;
};
// nparts: the partials a row of the producer -- fused: beam_nparts or hq_beam_nparts, else 1
static PlainBeamPlan plain_beam_plan(void* ws, size_t cap, int64_t Bd, int H, int64_t VT, int W, int max_len, bool step16, bool fused, int nparts,
                                     int32_t* backptr) {
    Workspace a(ws, cap);
    PlainBeamPlan p;
    const int64_t R = Bd * W;
    for (int k = 0; k < 2; ++k) { p.h[k] = a.take<float>((size_t)R * H); p.c[k] = a.take<float>((size_t)R * H); }
    for (int k = 0; k < 2; ++k) p.h16[k] = a.take<float>(step16 ? (size_t)R * H : 0);
    p.logits = a.take<float>(fused ? 0 : (size_t)R * VT);
    p.t.carve(a, Bd, W, max_len, nparts, fused, backptr);
    p.bytes = align_up(a.off, 256);
    return p;
}
// The search of both entries below, in the entry's `name`.  begin(p): the first state of every beam row into slot 0 (step16: and its term pairs
// into h16[0]).  Per step: the token-fed LSTM step from slot 0 into slot 1, the partials of the new state -- fused: gen_fused(p), the entry's
// producer; else the GEMM and the row kernel --, select, reorder.
template <class Begin, class GenFused>
static int plain_beam_decode(const char* name, int64_t Bd, int H, const float* table, int E, const float* w_ih, const float* w_hh, const float* b_ih,
                             const float* b_hh, const float* gate_fold, const void* whh_frag, bool step16, const float* gen_w, const float* gen_b, int64_t VT,
                             bool fused, int nparts, const int64_t* tgt2src, int64_t V, int64_t bos, int W, int max_len, void* workspace,
                             size_t workspace_bytes, int64_t* predictions, float* scores, int64_t* lengths, int32_t* backptr, hipStream_t st, Begin begin,
                             GenFused gen_fused) {
    const int64_t R = Bd * W;
    const PlainBeamPlan p = plain_beam_plan(workspace, workspace_bytes, Bd, H, VT, W, max_len, step16, fused, nparts, backptr);
    if (!workspace || p.bytes > workspace_bytes) {
        set_error("%s: workspace too small (%zu < %zu)", name, workspace_bytes, p.bytes);
        return NIR_ERR_WORKSPACE;
    }
    if (Bd == 0) return 0;
    const BeamTail& t = p.t;
    NIR_PROPAGATE(begin(p));
    NIR_PROPAGATE(launch_fill_i64(t.tgt, bos, R, st));
    NIR_PROPAGATE(t.begin(st));
    const LstmStepArgs s = beam_lstm_step_args(table, t.tgt, E, w_ih, w_hh, b_ih, b_hh, step16, gate_fold, whh_frag, R, H, p.h, p.c, p.h16);
    for (int step = 0; step < max_len; ++step) {
        NIR_PROPAGATE(launch_lstm_step(s, 1, st));
        NIR_PROPAGATE(fused ? gen_fused(p) : t.gen(false, p.h[1], H, gen_w, gen_b, nullptr, VT, p.logits, st));
        NIR_PROPAGATE(t.select(step, VT, tgt2src, V, st));
        NIR_PROPAGATE(t.reorder(step, H, p.h, p.c, step16 ? p.h16 : nullptr, st));
    }
    return t.end(predictions, scores, lengths, st);
}
// The stand-alone top-k of a fused producer: gen(p) writes its partials, nparts a row, into the workspace; one wave per row merges them.
template <class Gen>
static int beam_gen_topk_finish(void* workspace, size_t workspace_bytes, int nparts, int64_t rows, int W, float* top_val, int32_t* top_idx, float* lse,
                                hipStream_t st, Gen gen) {
    Workspace a(workspace, workspace_bytes);
    BeamPartials p;
    p.take(a, (size_t)nparts, rows, W, true);
    NIR_PROPAGATE(gen(p));
    hipLaunchKernelGGL(beam_topk_finish_kernel, dim3((unsigned)rows), dim3(64), 0, st, p.pval, p.pidx, p.pm, p.ps, nparts, rows, W, top_val, top_idx, lse);
    NIR_CHECK_LAUNCH("beam_topk_finish_kernel");
    return 0;
}
}  // namespace nir

extern "C" size_t nir_beam_plain_decode_workspace_bytes(int64_t Bd, int H, int64_t VT, int W, int max_len, int folded, int fused) {
    using namespace nir;
    if (Bd < 0 || H <= 0 || H % 4 || VT <= 0 || max_len <= 0 || !beam_dims_ok(W, VT)) return 0;
    const bool fuse = fused && gen_fusable(H, VT) && !tun(g_tun.exact_f32);
    return plain_beam_plan(nullptr, 0, Bd, H, VT, W, max_len, folded && H % 32 == 0 && !tun(g_tun.exact_f32), fuse, fuse ? beam_nparts(Bd * W, H, VT) : 1, nullptr)
        .bytes;
}

extern "C" int nir_beam_plain_decode(const float* dec_h, const float* dec_c, int64_t Bd, int H, const float* table, int64_t V, int E, const float* w_ih,
                                     const float* w_hh, const float* b_ih, const float* b_hh, const float* gen_w, const float* gen_b, int64_t VT,
                                     const int64_t* tgt2src, int64_t bos, int max_len, const float* gate_fold, const void* whh_frag, const void* gen_frag,
                                     int W, void* workspace, size_t workspace_bytes, int64_t* predictions, float* scores, int64_t* lengths, int32_t* backptr,
                                     nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(dec_h && dec_c && table && w_ih && w_hh && b_ih && b_hh && gen_w && predictions && scores && lengths, "beam_plain_decode: null pointer");
    NIR_REQUIRE(Bd >= 0 && H > 0 && E > 0 && V > 0 && VT > 0 && max_len > 0 && E % 4 == 0 && H % 4 == 0, "beam_plain_decode: bad dims");
    NIR_REQUIRE(bos >= 0 && bos < V, "beam_plain_decode: BOS id outside the vocabulary");
    NIR_REQUIRE(beam_dims_ok(W, VT), "beam_plain_decode: beam width outside [1, %d] or above the target vocabulary", NIR_BEAM_MAX_W);
    NIR_REQUIRE(Bd * NIR_BEAM_MAX_W < 0x7FFFFFFFLL && VT < 0x7FFFFFF0LL, "beam_plain_decode: too many decode rows or target tokens");
    const int64_t R = Bd * W;
    const bool step16 = gate_fold && whh_frag && H % 32 == 0 && !tun(g_tun.exact_f32), fused = s2s_gen_fused(gen_frag, H, VT);
    return plain_beam_decode(
        "beam_plain_decode", Bd, H, table, E, w_ih, w_hh, b_ih, b_hh, gate_fold, whh_frag, step16, gen_w, gen_b, VT, fused, fused ? beam_nparts(R, H, VT) : 1,
        tgt2src, V, bos, W, max_len, workspace, workspace_bytes, predictions, scores, lengths, backptr, st,
        [&](const PlainBeamPlan& p) { return launch_beam_repeat(dec_h, dec_c, Bd, R, H, p.h[0], p.c[0], step16 ? p.h16[0] : nullptr, nullptr, nullptr, st); },
        [&](const PlainBeamPlan& p) { return p.t.gen(true, p.h[1], H, gen_w, gen_b, gen_frag, VT, nullptr, st); });
}

// ---- HredQS (include/neuroir_hredqs_beam.h): the plain decoder's beam over Bd = B S source rows in the reference's pairing,
// the fast form's top-W on the split state the folded step leaves ---------------------------------------------------------------------------
extern "C" size_t nir_beam_hredqs_gen_topk_workspace_bytes(int64_t rows, int K, int64_t VT, int W) {
    using namespace nir;
    if (rows <= 0 || !gen_fusable(K, VT) || !beam_dims_ok(W, VT)) return 0;
    return beam_partials_bytes((size_t)hq_beam_nparts(rows, K, VT), rows, W, 4);
}

extern "C" int nir_beam_hredqs_gen_topk(const void* h16, int64_t rows, int K, const float* gen_b, const void* gen_frag, int64_t VT, int W, void* workspace,
                                        size_t workspace_bytes, float* top_val, int32_t* top_idx, float* lse, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(h16 && gen_frag && workspace && top_val && top_idx && lse, "beam_hredqs_gen_topk: null pointer");
    NIR_REQUIRE(rows >= 0 && rows < 0x7FFFFFFFLL, "beam_hredqs_gen_topk: bad dims");
    NIR_REQUIRE(gen_fusable(K, VT), "beam_hredqs_gen_topk: K must be a multiple of 32 in [32, 1024] and 0 < VT < 2^31 - 16");
    NIR_REQUIRE(beam_dims_ok(W, VT), "beam_hredqs_gen_topk: beam width outside [1, %d] or above VT", NIR_BEAM_MAX_W);
    if (rows == 0) return 0;
    if (workspace_bytes < nir_beam_hredqs_gen_topk_workspace_bytes(rows, K, VT, W)) {
        set_error("beam_hredqs_gen_topk: workspace too small");
        return NIR_ERR_WORKSPACE;
    }
    return beam_gen_topk_finish(workspace, workspace_bytes, hq_beam_nparts(rows, K, VT), rows, W, top_val, top_idx, lse, st, [&](const BeamPartials& p) {
        return launch_hq_beam_gen_topk((const _Float16*)h16, gen_frag, gen_b, VT, rows, K, W, p, st);
    });
}

extern "C" size_t nir_beam_hredqs_decode_workspace_bytes(int64_t B, int64_t S, int W, int max_len, const nir_hredqs_decoder_weights* w) {
    using namespace nir;
    if (!hq_weights_ok(w) || B < 0 || S < 0 || max_len <= 0 || !beam_dims_ok(W, w->VT)) return 0;
    const bool fast = hq_fast(w);
    return plain_beam_plan(nullptr, 0, B * S, w->H, w->VT, W, max_len, fast, fast, fast ? hq_beam_nparts(B * S * W, w->H, w->VT) : 1, nullptr).bytes;
}

extern "C" int nir_beam_hredqs_decode(const float* h_steps, const float* c_steps, int64_t B, int64_t S, const float* table, int64_t V, int E,
                                      const int64_t* tgt2src, int64_t bos, int max_len, const nir_hredqs_decoder_weights* w, int W, void* workspace,
                                      size_t workspace_bytes, int64_t* predictions, float* scores, int64_t* lengths, int32_t* backptr,
                                      nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(h_steps && c_steps && table && w && predictions && scores && lengths, "beam_hredqs_decode: null pointer");
    NIR_REQUIRE(hq_weights_ok(w), "beam_hredqs_decode: decoder weights incomplete, H not a multiple of 4 or VT outside (0, 2^31 - 16)");
    NIR_REQUIRE(B >= 0 && S >= 0 && max_len > 0 && V > 0 && E > 0 && E % 4 == 0, "beam_hredqs_decode: bad dims");
    NIR_REQUIRE(bos >= 0 && bos < V, "beam_hredqs_decode: BOS id outside the vocabulary");
    NIR_REQUIRE((w->rnn_gate_fold == nullptr) == (w->rnn_whh_frag == nullptr), "beam_hredqs_decode: rnn_gate_fold and rnn_whh_frag come together");
    NIR_REQUIRE(beam_dims_ok(W, w->VT), "beam_hredqs_decode: beam width outside [1, %d] or above the target vocabulary", NIR_BEAM_MAX_W);
    NIR_REQUIRE(B < 0x7FFFFFFFLL && S < 0x7FFFFFFFLL && B * S * NIR_BEAM_MAX_W < 0x7FFFFFFFLL, "beam_hredqs_decode: too many decode rows");
    const int H = w->H;
    const int64_t Bd = B * S, R = Bd * W, VT = w->VT;
    const bool fast = hq_fast(w);
    return plain_beam_decode(
        "beam_hredqs_decode", Bd, H, table, E, w->rnn_wih, w->rnn_whh, w->rnn_bih, w->rnn_bhh, w->rnn_gate_fold, w->rnn_whh_frag, fast, w->gen_w, w->gen_b, VT, fast,
        fast ? hq_beam_nparts(R, H, VT) : 1, tgt2src, V, bos, W, max_len, workspace, workspace_bytes, predictions, scores, lengths, backptr, st,
        [&](const PlainBeamPlan& p) {
            // pairing, repeat and split in one launch: every beam of source row i starts from step i / B of session i % B
            return launch_hq_beam_begin(h_steps, c_steps, B, S, H, R, p.h[0], p.c[0], fast ? reinterpret_cast<_Float16*>(p.h16[0]) : nullptr, st);
        },
        [&](const PlainBeamPlan& p) {
            return launch_hq_beam_gen_topk(reinterpret_cast<const _Float16*>(p.h16[1]), w->gen_frag, w->gen_b, VT, R, H, W, p.t.part, st);
        });
}

extern "C" size_t nir_beam_gen_topk_workspace_bytes(int64_t rows, int K, int64_t VT, int W, int fused) {
    using namespace nir;
    if (rows <= 0 || K <= 0 || !beam_dims_ok(W, VT)) return 0;
    if (!fused) return (size_t)rows * VT * sizeof(float) + 256;
    if (!gen_fusable(K, VT)) return 0;
    return beam_partials_bytes((size_t)beam_nparts(rows, K, VT), rows, W, 4);
}

extern "C" int nir_beam_gen_topk(const float* x, int64_t rows, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT, int W,
                                 void* workspace, size_t workspace_bytes, float* top_val, int32_t* top_idx, float* lse, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(x && gen_w && workspace && top_val && top_idx && lse, "beam_gen_topk: null pointer");
    NIR_REQUIRE(rows >= 0 && rows < 0x7FFFFFFFLL && K > 0 && K % 4 == 0 && VT > 0, "beam_gen_topk: bad dims");
    NIR_REQUIRE(beam_dims_ok(W, VT), "beam_gen_topk: beam width outside [1, %d] or above VT", NIR_BEAM_MAX_W);
    const bool fused = s2s_gen_fused(gen_frag, K, VT);
    NIR_REQUIRE(fused || VT < 0x7FFFFFFFLL, "beam_gen_topk: VT too large for the GEMM path");
    if (rows == 0) return 0;
    if (workspace_bytes < nir_beam_gen_topk_workspace_bytes(rows, K, VT, W, fused)) {
        set_error("beam_gen_topk: workspace too small");
        return NIR_ERR_WORKSPACE;
    }
    if (fused)
        return beam_gen_topk_finish(workspace, workspace_bytes, beam_nparts(rows, K, VT), rows, W, top_val, top_idx, lse, st, [&](const BeamPartials& p) {
            return launch_beam_gen_topk(x, gen_frag, gen_b, VT, rows, K, W, p, st);
        });
    Workspace a(workspace, workspace_bytes);
    float* logits = a.take<float>((size_t)rows * VT);
    NIR_PROPAGATE(launch_linear(x, K, nullptr, nullptr, 0, 0, 0, gen_w, K, gen_b, nullptr, logits, VT, rows, (int)VT, K, NIR_ACT_NONE, st));
    return launch_beam_row_topk(logits, VT, rows, W, top_val, top_idx, lse, st);
}

extern "C" int nir_beam_select(const float* top_val, const int32_t* top_idx, const float* lse, int64_t B, int W, int64_t VT, const int64_t* tgt2src,
                               int64_t V, float* cum, int32_t* finished, int32_t* backptr, int32_t* token, int64_t* next_ids, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(top_val && top_idx && lse && cum && finished && backptr && token && next_ids, "beam_select: null pointer");
    NIR_REQUIRE(B >= 0 && B * NIR_BEAM_MAX_W < 0x7FFFFFFFLL && V > 0, "beam_select: bad dims");
    NIR_REQUIRE(beam_dims_ok(W, VT), "beam_select: beam width outside [1, %d] or above VT", NIR_BEAM_MAX_W);
    if (B == 0) return 0;
    return launch_beam_select(top_val, top_idx, lse, nullptr, 1, B, W, VT, tgt2src, V, cum, finished, backptr, token, next_ids, (hipStream_t)stream);
}

extern "C" int nir_beam_reorder(const int32_t* backptr, int64_t B, int W, int H, const float* h_in, float* h_out, const float* c_in, float* c_out,
                                const void* h16_in, void* h16_out, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(backptr && h_in && h_out, "beam_reorder: null pointer");
    NIR_REQUIRE((c_in == nullptr) == (c_out == nullptr) && (h16_in == nullptr) == (h16_out == nullptr), "beam_reorder: a state needs its input and its output");
    NIR_REQUIRE(B >= 0 && B * NIR_BEAM_MAX_W < 0x7FFFFFFFLL && H > 0 && H % 4 == 0 && (!h16_in || H % 8 == 0), "beam_reorder: bad dims");
    NIR_REQUIRE(W >= 1 && W <= NIR_BEAM_MAX_W, "beam_reorder: beam width outside [1, %d]", NIR_BEAM_MAX_W);
    NIR_REQUIRE(h_in != h_out && (!c_in || c_in != c_out) && (!h16_in || h16_in != h16_out), "beam_reorder: an output aliases its input");
    if (B == 0) return 0;
    return launch_beam_reorder(backptr, B, W, H, h_in, h_out, c_in, c_out, h16_in, h16_out, (hipStream_t)stream);
}

extern "C" size_t nir_beam_seq2seq_decode_workspace_bytes(int64_t B, int QL, int W, int max_len, const nir_seq2seq_decoder_weights* w) {
    return nir::beam_decode_workspace_bytes(B, QL, W, max_len, w, nir::S2S_CELL_LSTM);
}
extern "C" int nir_beam_seq2seq_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, int W,
                                       const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                                       const nir_seq2seq_decoder_weights* w, void* workspace, size_t workspace_bytes, int64_t* predictions, float* scores,
                                       int64_t* lengths, float* attentions, int32_t* backptr, nir_stream_t stream) {
    return nir::s2s_beam_decode(dec_h, dec_c, memory_bank, source_len, B, QL, W, table, V, E, tgt2src, bos, max_len, w, workspace, workspace_bytes,
                                predictions, scores, lengths, attentions, backptr, nir::S2S_CELL_LSTM, (hipStream_t)stream);
}
extern "C" size_t nir_beam_seq2seq_gru_decode_workspace_bytes(int64_t B, int QL, int W, int max_len, const nir_seq2seq_decoder_weights* w) {
    return nir::beam_decode_workspace_bytes(B, QL, W, max_len, w, nir::S2S_CELL_GRU);
}
extern "C" int nir_beam_seq2seq_gru_decode(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, int W,
                                           const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                                           const nir_seq2seq_decoder_weights* w, void* workspace, size_t workspace_bytes, int64_t* predictions,
                                           float* scores, int64_t* lengths, float* attentions, int32_t* backptr, nir_stream_t stream) {
    return nir::s2s_beam_decode(dec_h, nullptr, memory_bank, source_len, B, QL, W, table, V, E, tgt2src, bos, max_len, w, workspace, workspace_bytes,
                                predictions, scores, lengths, attentions, backptr, nir::S2S_CELL_GRU, (hipStream_t)stream);
}

// ---- the copy generator's beam (include/neuroir_acg_beam.h) ---------------------------------------------------------------------------------------
extern "C" size_t nir_acg_beam_gen_select_workspace_bytes(int64_t rows, int K, int64_t VT, int W, int fused) {
    using namespace nir;
    if (rows <= 0 || K <= 0 || !beam_dims_ok(W, VT)) return 0;
    if (fused && !gen_fusable(K, VT)) return 0;
    const size_t parts = fused ? (size_t)beam_nparts(rows, K, VT) : 1;
    return (fused ? 0 : align_up((size_t)rows * VT * sizeof(float), 256)) + beam_partials_bytes(parts, rows, W, 5);
}

namespace nir {
// nir_acg_beam_gen_select; logit_targets (the sampler's top-k form, csrc/sample.hip): in the plain form a collapse target's logit is read from the
// GEMM's workspace logits instead of the wave's row dot.  The beam's entry passes false.
int acg_beam_gen_select_rows(const float* o, int64_t rows, int64_t nsrc, int K, const float* gen_w, const float* gen_b, const void* gen_frag,
                             int64_t VT, int W, const float* copy_w, const float* copy_b, const float* copy_attn, int64_t attn_stride,
                             const int64_t* source_len, int QL, const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src, int CV,
                             void* workspace, size_t workspace_bytes, float* top_val, int32_t* top_idx, nir_stream_t stream, bool logit_targets) {
    NIR_REQUIRE(o && gen_w && copy_w && copy_b && copy_attn && source_len && src_map_idx && ext2tgt && ext2src && workspace && top_val && top_idx,
                "acg_beam_gen_select: null pointer");
    NIR_REQUIRE(rows >= 0 && rows < 0x7FFFFFFFLL && nsrc >= 0 && (rows == 0 || (nsrc > 0 && nsrc <= rows)) && K > 0 && K % 4 == 0 && VT > 0 &&
                    attn_stride >= QL,
                "acg_beam_gen_select: bad dims");
    NIR_REQUIRE(beam_dims_ok(W, VT), "acg_beam_gen_select: beam width outside [1, %d] or above VT", NIR_BEAM_MAX_W);
    NIR_REQUIRE(acg_beam_dims_ok(QL, CV, VT), "acg_beam_gen_select: QL outside [1, 4096], CV outside [2, %d], or VT + CV too large", ACG_MAX_CV);
    const bool fused = s2s_gen_fused(gen_frag, K, VT);
    if (rows == 0) return 0;
    if (workspace_bytes < nir_acg_beam_gen_select_workspace_bytes(rows, K, VT, W, fused)) {
        set_error("acg_beam_gen_select: workspace too small");
        return NIR_ERR_WORKSPACE;
    }
    Workspace a(workspace, workspace_bytes);
    const size_t parts = fused ? (size_t)beam_nparts(rows, K, VT) : 1;
    float* logits = a.take<float>(fused ? 0 : (size_t)rows * VT);
    BeamPartials p;
    p.take(a, parts, rows, W, true);
    return launch_acg_beam_gen_select(o, rows, nsrc, K, gen_w, gen_b, fused ? gen_frag : nullptr, VT, W, logits, p, copy_w, copy_b, copy_attn, attn_stride,
                                      source_len, QL, src_map_idx, ext2tgt, CV, nullptr, top_val, top_idx, (hipStream_t)stream, logit_targets);
}
}  // namespace nir

extern "C" int nir_acg_beam_gen_select(const float* o, int64_t rows, int64_t nsrc, int K, const float* gen_w, const float* gen_b, const void* gen_frag,
                                       int64_t VT, int W, const float* copy_w, const float* copy_b, const float* copy_attn, int64_t attn_stride,
                                       const int64_t* source_len, int QL, const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src, int CV,
                                       void* workspace, size_t workspace_bytes, float* top_val, int32_t* top_idx, nir_stream_t stream) {
    return nir::acg_beam_gen_select_rows(o, rows, nsrc, K, gen_w, gen_b, gen_frag, VT, W, copy_w, copy_b, copy_attn, attn_stride, source_len, QL, src_map_idx,
                                         ext2tgt, ext2src, CV, workspace, workspace_bytes, top_val, top_idx, stream, false);
}

extern "C" int nir_acg_beam_select(const float* top_val, const int32_t* top_idx, const float* lse, int64_t B, int W, int64_t VT, int CV,
                                   const int64_t* tgt2src, const int64_t* ext2src, int64_t V, float* cum, int32_t* finished, int32_t* backptr,
                                   int32_t* token, int64_t* next_ids, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(top_val && top_idx && ext2src && cum && finished && backptr && token && next_ids, "acg_beam_select: null pointer");
    NIR_REQUIRE(B >= 0 && B * NIR_BEAM_MAX_W < 0x7FFFFFFFLL && V > 0, "acg_beam_select: bad dims");
    NIR_REQUIRE(beam_dims_ok(W, VT), "acg_beam_select: beam width outside [1, %d] or above VT", NIR_BEAM_MAX_W);
    NIR_REQUIRE(acg_beam_dims_ok(1, CV, VT), "acg_beam_select: CV outside [2, %d], or VT + CV too large", ACG_MAX_CV);
    if (B == 0) return 0;
    return launch_acg_beam_select(top_val, top_idx, lse, B, W, VT, CV, tgt2src, ext2src, V, cum, finished, backptr, token, next_ids, (hipStream_t)stream);
}

extern "C" size_t nir_acg_beam_decode_workspace_bytes(int64_t B, int QL, int CV, int W, int max_len, const nir_seq2seq_decoder_weights* w,
                                                      const nir_acg_copy_weights* cw) {
    if (!cw) return 0;
    nir::AcgDecode g{cw, nullptr, nullptr, nullptr, CV};
    return nir::beam_decode_workspace_bytes(B, QL, W, max_len, w, nir::S2S_CELL_LSTM, &g);
}
extern "C" int nir_acg_beam_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL,
                                   const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                                   const nir_seq2seq_decoder_weights* w, const nir_acg_copy_weights* cw, const int64_t* src_map_idx, const int64_t* ext2tgt,
                                   const int64_t* ext2src, int CV, int W, void* workspace, size_t workspace_bytes, int64_t* predictions, float* scores,
                                   int64_t* lengths, float* attentions, int32_t* backptr, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(cw, "acg_beam_decode: null copy weights");
    AcgDecode g{cw, src_map_idx, ext2tgt, ext2src, CV};
    return s2s_beam_decode(dec_h, dec_c, memory_bank, source_len, B, QL, W, table, V, E, tgt2src, bos, max_len, w, workspace, workspace_bytes, predictions,
                           scores, lengths, attentions, backptr, S2S_CELL_LSTM, (hipStream_t)stream, &g);
}
extern "C" size_t nir_acg_beam_gru_decode_workspace_bytes(int64_t B, int QL, int CV, int W, int max_len, const nir_seq2seq_decoder_weights* w,
                                                          const nir_acg_copy_weights* cw) {
    if (!cw) return 0;
    nir::AcgDecode g{cw, nullptr, nullptr, nullptr, CV};
    return nir::beam_decode_workspace_bytes(B, QL, W, max_len, w, nir::S2S_CELL_GRU, &g);
}
extern "C" int nir_acg_beam_gru_decode(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, const float* table,
                                       int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w,
                                       const nir_acg_copy_weights* cw, const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src, int CV,
                                       int W, void* workspace, size_t workspace_bytes, int64_t* predictions, float* scores, int64_t* lengths,
                                       float* attentions, int32_t* backptr, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(cw, "acg_beam_decode: null copy weights");
    AcgDecode g{cw, src_map_idx, ext2tgt, ext2src, CV};
    return s2s_beam_decode(dec_h, nullptr, memory_bank, source_len, B, QL, W, table, V, E, tgt2src, bos, max_len, w, workspace, workspace_bytes, predictions,
                           scores, lengths, attentions, backptr, S2S_CELL_GRU, (hipStream_t)stream, &g);
}
