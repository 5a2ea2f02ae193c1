// The generator kernel of the greedy attention decoders (csrc/seq2seq.hip: arg-max; csrc/acg.hip: arg-max + softmax statistics) and its
// launch geometry.  One template: STATS = false is the Seq2seq kernel, STATS = true additionally keeps the online-softmax sum of every row.
#pragma once
#include <mutex>
#include "decode_common.hpp"

namespace nir {

// ---- generator + bias + arg-max: logits[b, v] = x[b, :] . W[v, :] + bias[v] never leave the chip --------------------------------
// W [VT, K] (K = 32 .. 1024, a multiple of 32) arrives as two fp16 term planes in MFMA A-fragment order (s2s_gen_frag_kernel):
//   frag[vt][ks][term][lane][8],  element (lane, j) = W[16 vt + (lane & 15)][32 ks + 8 (lane >> 4) + j],  rows past VT are zero.
// A workgroup stages 16 NBT decode rows as two fp16 planes in LDS ([2][16 NBT][K + 8] halves: NBT = 4 up to K = 512 -- 133 KB -- and 2
// beyond -- 132 KB at K = 1024; gfx950 has 160 KB) and walks its range of vocabulary tiles, a wave one tile at a time.  A tile's k-steps
// go in chunks of GEN_KC: the fragments of the next chunk (or of the next tile's first chunk) are requested before the MFMAs of the
// current one are issued.  Three v_mfma_f32_16x16x32_f16 per product block (hi hi -> acc; lo hi, hi lo -> acx; result acc + 2^-11 acx),
// the bias is added in fp32 before the comparison, `>` in ascending index order keeps the first index on ties.  Every wave writes one
// (value, index) partial per decode row; argmax_finish_kernel reduces them.
//
// STATS (csrc/acg.hip, the copy generator: modules/copy_generator.py:78-80): the logit of v == PAD (0) is replaced by -1e-20f before the comparison,
// and every lane keeps the online-softmax sum of its rows next to the running maximum -- sum_v exp(y_v - best), rescaled when best moves (one
// rescale and four exponentials per tile and row) -- so a partial is (best, index, sum) and softmax statistics need no [B, VT] logits either.
// STATS = false compiles to the arg-max kernel alone (psum is not read).
template <int NBT, bool STATS = false>
__global__ __launch_bounds__(256, 1) void s2s_gen_argmax_kernel(const float* __restrict__ x, const _Float16* __restrict__ wfrag,
                                                                const float* __restrict__ bias, int64_t VT, int64_t ntiles, int64_t Bd, int K,
                                                                int nvr, float* __restrict__ pval, int* __restrict__ pidx,
                                                                float* __restrict__ psum) {
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
    float rsum[NBT];
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) rsum[bt] = 0.f;
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
    const _Float16* bp0 = s2s_sm + c16 * LD + 8 * g4;
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
        if (STATS && c == NCH - 1) {
            const int64_t v0 = t * 16 + 4 * g4;
            float bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) bv[r] = (bias && v0 + r < VT) ? bias[v0 + r] : 0.f;
#pragma unroll
            for (int bt = 0; bt < NBT; ++bt) {
                float y[4];
                float m = best[bt];
                int mi = bidx[bt];
#pragma unroll
                for (int r = 0; r < 4; ++r) {                                 // ascending in r: '>' keeps the first index on ties
                    y[r] = fmaf(acx[bt][r], SPLIT2_INV, acc[bt][r]) + bv[r];
                    if (v0 + r == 0) y[r] = -1e-20f;                          // PAD: the reference assigns this constant behind the linear
                    if (v0 + r >= VT) y[r] = -INFINITY;                       // padded tile rows: never win, add exp(-inf) = 0
                    if (y[r] > m) { m = y[r]; mi = (int)(v0 + r); }
                }
                if (m > -INFINITY) {                                          // (v0 < VT for every tile walked, so only NaN logits skip this)
                    rsum[bt] = rsum[bt] * __expf(best[bt] - m) + ((__expf(y[0] - m) + __expf(y[1] - m)) + (__expf(y[2] - m) + __expf(y[3] - m)));
                    best[bt] = m;
                    bidx[bt] = mi;
                }
            }
        }
        if (!STATS && c == NCH - 1) {
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
    // lanes l, l + 16, l + 32, l + 48 hold the same decode row: combine (first index wins ties), then one partial per wave and row
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) {
#pragma unroll
        for (int sh = 16; sh <= 32; sh <<= 1) {
            const float ov = __shfl_xor(best[bt], sh);
            const int oi = __shfl_xor(bidx[bt], sh);
            if (STATS) {                                                      // both lanes of a pair form the same sum: a + b commutes
                const float os = __shfl_xor(rsum[bt], sh);
                const float m = fmaxf(ov, best[bt]);
                rsum[bt] = m > -INFINITY ? rsum[bt] * __expf(best[bt] - m) + os * __expf(ov - m) : 0.f;
            }
            if (ov > best[bt] || (ov == best[bt] && oi < bidx[bt])) { best[bt] = ov; bidx[bt] = oi; }
        }
        const int64_t b = b0 + bt * 16 + c16;
        if (g4 == 0 && b < Bd) {
            const int64_t slot = ((int64_t)vr * 4 + wave) * Bd + b;
            pval[slot] = best[bt];
            pidx[slot] = bidx[bt];
            if (STATS) psum[slot] = rsum[bt];
        }
    }
}

// The launch of either form: nvr vocabulary ranges (s2s_nvr) x the row blocks of Bd, *nparts = 4 nvr partials a row.  name: the label of the
// profile and of the launch check (s2s_gen_argmax_kernel, s2s_gen_stats_kernel).  GEN_KC and the geometry (gen_nbt, gen_lds, gen_fusable,
// s2s_nvr) live in decode_common.hpp, shared with the generator kernels of csrc/hredqs.hip and csrc/beam.hip.
template <bool STATS>
static int launch_gen_argmax_partials(const char* name, const float* x, const void* frag, const float* bias, int64_t VT, int64_t Bd, int K, float* pval,
                                      int* pidx, float* psum, int* nparts, hipStream_t st) {
    const int64_t ntiles = (VT + 15) / 16;
    const int nbt = gen_nbt(K), nvr = s2s_nvr(Bd, K, ntiles);
    const int64_t rb = (Bd + 16 * nbt - 1) / (16 * nbt);
    const size_t lds = gen_lds(K);
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute((const void*)s2s_gen_argmax_kernel<4, STATS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds(512));
        (void)hipFuncSetAttribute((const void*)s2s_gen_argmax_kernel<2, STATS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds(1024));
    });
    {
        ProfScope ps(prof_shape_name(name, (long long)Bd, (long long)VT, K), st);
        if (nbt == 4)
            hipLaunchKernelGGL((s2s_gen_argmax_kernel<4, STATS>), dim3((unsigned)(nvr * rb)), dim3(256), lds, st, x, (const _Float16*)frag, bias, VT, ntiles, Bd,
                               K, nvr, pval, pidx, psum);
        else
            hipLaunchKernelGGL((s2s_gen_argmax_kernel<2, STATS>), dim3((unsigned)(nvr * rb)), dim3(256), lds, st, x, (const _Float16*)frag, bias, VT, ntiles, Bd,
                               K, nvr, pval, pidx, psum);
    }
    NIR_CHECK_LAUNCH(name);
    *nparts = nvr * 4;
    return 0;
}
// the fused generator runs (arg-max, statistics or top-k alike): the fragments are given, the shape has a fused form, tunable exact_f32 is off
static inline bool s2s_gen_fused(const void* gen_frag, int K, int64_t VT) { return gen_frag != nullptr && gen_fusable(K, VT) && !tun(g_tun.exact_f32); }

// ---- ACG: the copy generator behind the Seq2seq step (csrc/acg.hip) ----------------------------------------------------------------------
constexpr float ACG_PAD_LOGIT = -1e-20f;              // copy_generator.py:79: logits[:, :, PAD] = -eps
constexpr int ACG_MAX_CV = 1024;                      // dictionary slots of a row kept in LDS by acg_select_kernel (4 rows x 3 arrays x 4 KB)
static inline bool acg_dims_ok(int QL, int CV) { return QL > 0 && QL <= 4096 && CV >= 2 && CV <= ACG_MAX_CV; }
struct AcgDecode {
    const nir_acg_copy_weights* cw;
    const int64_t *src_map_idx, *ext2tgt, *ext2src;  // [B,QL], [B,CV], [B,CV]
    int CV;
};
bool acg_weights_ok(const nir_seq2seq_decoder_weights* w, const AcgDecode* g);   // csrc/seq2seq.hip: the copy weights the attention type needs
// generator statistics (fused: gen_frag != NULL, the STATS kernel above; plain: GEMM into `logits` + acg_row_stats_kernel) + acg_select_kernel
int launch_acg_gen_select(const float* o, int64_t B, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT, float* logits,
                          float* pval, int* pidx, float* psum, const float* copy_w, const float* copy_b, const float* attn, int64_t attn_stride,
                          const int64_t* lens, int QL, const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src, int CV,
                          const int64_t* tgt2src, int64_t V, int64_t* pred, int64_t pstride, int64_t* tgt, hipStream_t st);
// csrc/seq2seq.hip, shared with the beam search of csrc/beam.hip: the weight checks, the two decisions every decode makes once -- the fused
// generator (s2s_gen_fused above, on the pack's fields) and the fp16-term cell step (both packs given, H a multiple of 32, tunable exact_f32
// off) -- and the attention launch (nsrc: decode row i attends over source row i % nsrc; 0 = one source row per decode row)
bool s2s_weights_ok(const nir_seq2seq_decoder_weights* w);
bool s2s_fused(const nir_seq2seq_decoder_weights* w);
bool s2s_step16(const nir_seq2seq_decoder_weights* w);
int launch_attend(const float* q, const float* h, const float* mem, const float* sb, const float* v, const int64_t* lens, int64_t B, int QL, int H,
                  int mlp, float* cat, float* attn, int64_t attn_stride, hipStream_t st, int64_t nsrc = 0);

// ACG's copy attention, once for the greedy, beam and sampling decodes.  With reuse_copy_attn it is the stepper's attention row as it stands (own
// stays false: nothing is carved or launched).  Otherwise a second attention in the forms of the stepper's, whose query is the attentional output
// ah [rows, H] (its own cat and linear_out take no part in the value): the score bank over the nsrc source rows once per decode, per step the
// (mlp) query GEMM and launch_attend into cattn [rows, QL].
struct AcgCopyAttn {
    float *csb = nullptr, *cq = nullptr, *ccat = nullptr, *cattn = nullptr;
    bool own = false;
    // own_copy_attn: the four buffers, in this order
    void carve(Workspace& a, int64_t rows, int64_t nsrc, int QL, int H, int attn_type) {
        own = true;
        csb = a.take<float>(attn_type == NIR_S2S_ATTN_DOT ? 0 : (size_t)nsrc * QL * H);
        cq = a.take<float>(attn_type == NIR_S2S_ATTN_MLP ? (size_t)rows * H : 0);
        ccat = a.take<float>((size_t)rows * 2 * H);
        cattn = a.take<float>((size_t)rows * QL);
    }
    int prepare(const nir_acg_copy_weights* cw, const float* memory_bank, int64_t nsrc, int QL, int H, int attn_type, hipStream_t st) const {
        if (!own || attn_type == NIR_S2S_ATTN_DOT) return 0;
        return launch_linear(memory_bank, H, nullptr, nullptr, 0, 0, 0, attn_type == NIR_S2S_ATTN_MLP ? cw->attn_ctx_w : cw->attn_in_wt, H, nullptr, nullptr, csb, H,
                             nsrc * QL, H, H, NIR_ACT_NONE, st);
    }
    // *ca / *ca_stride: in, the stepper's attention rows of this step; out, the copy attention's
    int step(const nir_acg_copy_weights* cw, const float* ah, int64_t rows, int64_t nsrc, const float* memory_bank, const int64_t* source_len, int QL, int H,
             int attn_type, const float** ca, int64_t* ca_stride, hipStream_t st) const {
        if (!own) return 0;
        const bool mlp = attn_type == NIR_S2S_ATTN_MLP;
        if (mlp) NIR_PROPAGATE(launch_linear(ah, H, nullptr, nullptr, 0, 0, 0, cw->attn_query_w, H, cw->attn_query_b, nullptr, cq, H, rows, H, H, NIR_ACT_NONE, st));
        NIR_PROPAGATE(launch_attend(mlp ? cq : ah, ah, memory_bank, attn_type == NIR_S2S_ATTN_DOT ? memory_bank : csb, cw->attn_v, source_len, rows, QL, H, mlp,
                                    ccat, cattn, QL, st, nsrc));
        *ca = cattn;
        *ca_stride = QL;
        return 0;
    }
};

// ---- the attention-decoder step, once: cell -> (mlp: query GEMM) -> attention -> linear_out -----------------------------------------------------
// The greedy decodes of Seq2seq and ACG (s2s_decode) and the beam search (csrc/beam.hip) are this stepper with a tail each behind linear_out:
// arg-max, the copy generator's select, or top-k + select + reorder.  `rows` decode rows over `nsrc` source rows (greedy: B and B; beam: B W and B,
// decode row i reads the banks of source row i % nsrc).  cell: the decoder's recurrence, S2S_CELL_LSTM (launch_lstm_step) or S2S_CELL_GRU
// (launch_gru_step: no cell state, dec_c and the c buffers unused).
constexpr int S2S_CELL_LSTM = 0, S2S_CELL_GRU = 1;
struct S2sStepBufs {                                  // the stepper's part of a decode's workspace plan
    float *sb, *h[2], *c[2], *h16[2], *qh, *cat, *ah, *logits, *gru;       // (logits: the plain generator of the tails; gru: the plain GRU step's gates)
    int64_t* tgt;                                     // [rows] the token ids the next step reads
};
// takes sb .. logits, in this order; h16: with the fp16 term pairs of the state (the greedy plan always, the beam plan with the fp16-term step
// only).  tgt and gru are taken by the caller's plan where they always lay among its own buffers, so every workspace keeps its layout.
S2sStepBufs s2s_step_bufs(Workspace& a, int64_t rows, int64_t nsrc, int QL, int H, int64_t VT, int attn_type, bool fused, int cell, bool h16);
struct S2sStepper {
    const char* name;                                 // the entry's name: the prefix of every message
    const nir_seq2seq_decoder_weights* w;
    int cell;
    const float *table, *memory_bank;
    const int64_t* source_len;
    int64_t V, rows, nsrc;
    int E, QL;
    hipStream_t st;
    bool fused = false, step16 = false;               // set by check()
    S2sStepBufs b{};                                  // set by the caller from its plan, in front of prepare()
    const float* sb = nullptr;                        // the bank the scores are taken against (prepare())
    LstmStepArgs a;
    GruStepArgs ga;
    // the argument checks of a decode entry, in its name; outputs: the entry's own output pointers are all given
    int check(const float* dec_h, const float* dec_c, bool outputs, int64_t bos, int max_len);
    // the score-bank GEMM, the BOS fill, the cell's arguments and, with the fp16-term step, dec_h as term pairs into h16first
    int prepare(const float* dec_h, int64_t bos, float* h16first);
    // one step from (hp, cp, h16prev) into (hn, cn, h16next); attention row i at attn_out + i * attn_stride.  Behind it b.ah [rows, H] is the
    // attentional output and b.tgt still the ids the step read: the tail writes the next ones
    int step(const float* hp, const float* cp, float* hn, float* cn, const float* h16prev, float* h16next, float* attn_out, int64_t attn_stride);
};
// csrc/seq2seq.hip: the greedy decode of Seq2seq (acg == NULL) and of ACG
size_t s2s_decode_workspace_bytes(int64_t B, int QL, const nir_seq2seq_decoder_weights* w, const AcgDecode* acg, int cell);
int s2s_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, const float* table,
               int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w, void* workspace,
               size_t workspace_bytes, int64_t* predictions, float* attentions, const AcgDecode* acg, int cell, hipStream_t st);

}  // namespace nir
