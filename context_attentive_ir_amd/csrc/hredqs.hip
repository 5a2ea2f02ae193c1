// HredQS.decode -- greedy decoding of the hierarchical recurrent encoder-decoder (neuroir/recommender/hredqs.py:169-230; Decoder with
// attn_type 'none': decoders/decoder.py:120-177).  A batch of B sessions of S queries decodes R = B S rows, one per session prefix.
//
// Once per decode: the R initial states in the reference's pairing (decode row r starts from session step r / B of session r % B)
//                                                                                                   hq_pair_kernel
// Per step, for all R rows at once:
//   fast:  (h,c) = LSTM(emb(tok), (h,c)), tok read from the previous step's arg-max keys             lstm_step16_kernel (launch_lstm_step)
//          key = max_v argmax_key((W_g h + b_g)_v, v)                                                 hq_gen_argmax_kernel
//   plain: fp32 LSTM step, fp32 generator GEMM, arg-max + target -> source map                       lstm_step_kernel, GEMM, argmax_map_kernel
// Behind the loop (fast): keys [max_len][R][ARGMAX_KEY_BUCKETS] -> predictions                        hq_keys_decode_kernel
// Everything is enqueued on the caller's stream; no host synchronisation, no allocation, no float atomics (the 64-bit integer atomicMax
// is order-independent: the same inputs give the same bits).
#include <algorithm>
#include <mutex>
#include "decode_common.hpp"

namespace nir {

// ---- the initial states in pairing order ---------------------------------------------------------------------------------------------------------
// hs / cs [B, S, H] (session b, step s at row b S + s) -> h0 / c0 [R, H]: row r = the state of step r / B of session r % B; h16 (optional):
// h0 as the fp16 term pairs of the folded step, [row][H/8][2][8] (h16_pack_kernel's format).
__global__ void hq_pair_kernel(const float* __restrict__ hs, const float* __restrict__ cs, int64_t B, int64_t S, int H, float* __restrict__ h0,
                               float* __restrict__ c0, _Float16* __restrict__ h16) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B * S * H) return;
    const int64_t r = e / H;
    const int k = (int)(e - r * H);
    const int64_t src = ((r % B) * S + r / B) * H + k;
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

// ---- generator + bias + arg-max on the split state ------------------------------------------------------------------------------------------------
// W [VT, K] (K = 32 .. 1024, a multiple of 32) arrives as nir_seq2seq_pack_gen_frag leaves it: two fp16 term planes in MFMA A-fragment order,
//   frag[vt][ks][term][lane][8],  element (lane, j) = W[16 vt + (lane & 15)][32 ks + 8 (lane >> 4) + j],  rows past VT are zero.
// The decode rows arrive ALREADY split, as the folded LSTM step writes them (h16 [row][K/8][2 terms][8]): staging is a 16-byte copy per
// (row, k-group, term) into two LDS planes [2][16 NBT][K + 8] halves (NBT = 4 up to K = 512 -- 133 KB -- and 2 beyond -- 132 KB at K = 1024),
// no conversion.  A workgroup then walks its range of vocabulary tiles, a wave one tile at a time, the fragments of the next chunk of k-steps
// requested before the MFMAs of the current one (the product of s2s_gen_argmax_kernel: hi hi -> acc; lo hi, hi lo -> acx; acc + 2^-11 acx,
// bias added in fp32, `>` in ascending index order keeps the first index on ties).
// The end is keyed: the four waves' winners meet in LDS, then ONE 64-bit atomicMax per workgroup and decode row on keys[row][vr % BUCKETS].
//
// Grid: nrb row blocks x nvr vocabulary ranges, R = 128 .. 768 rows is 4 .. 24 row blocks at K = 1024.  All row blocks of a range read the
// same fragments, so they are placed to run TOGETHER and on ONE L2: blocks with equal blockIdx % 8 share an XCD and are dispatched in
// ascending order there, so with j = blockIdx / 8 the row block is j % nrb and the range (j / nrb) * 8 + blockIdx % 8 (nvr a multiple of 8).
// A range's fragments then come from HBM once and from that XCD's L2 for the other row blocks.  With nvr no multiple of 8 the row block is
// blockIdx % nrb: still adjacent in dispatch order, sharing through the Infinity Cache only.  The mapping is a speed choice: any placement
// gives the same keys.  (GEN_KC and the grid helpers gen_nbt / gen_lds / hq_nvr live in decode_common.hpp, shared with the other generator kernels.)
template <int NBT>
__global__ __launch_bounds__(256, 1) void hq_gen_argmax_kernel(const _Float16* __restrict__ h16, const _Float16* __restrict__ wfrag,
                                                               const float* __restrict__ bias, int64_t VT, int64_t ntiles, int64_t R, int K, int nvr,
                                                               int nrb, unsigned long long* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) _Float16 hq_sm[];            // [2 terms][ROWS][LD]
    constexpr int ROWS = 16 * NBT;
    const int LD = K + 8, KS = K / 32, Q = K / 4;                               // Q: 16-byte chunks of a row (k-group, term)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g4 = lane >> 4;
    int vr, rb;
    if (nvr % 8 == 0) {
        const int j = (int)(blockIdx.x >> 3);
        rb = j % nrb;
        vr = (j / nrb) * 8 + (int)(blockIdx.x & 7);
    } else {
        rb = (int)(blockIdx.x % nrb);
        vr = (int)(blockIdx.x / nrb);
    }
    const int64_t b0 = (int64_t)rb * ROWS;
    const int64_t per_wg = (ntiles + nvr - 1) / nvr;
    const int64_t t_lo = (int64_t)vr * per_wg, t_hi = min(ntiles, t_lo + per_wg);
    {
        // stage this workgroup's decode rows (zero rows past R).  The loads of HQ_SB trips are issued before the first is written (unconditional,
        // from a clamped row: a branch around a load puts an s_waitcnt vmcnt(0) at its join)
        constexpr int HQ_SB = 8;
        const int total = ROWS * Q;                                             // a multiple of 256
        for (int e0 = tid; e0 < total; e0 += 256 * HQ_SB) {
            uint4 sv[HQ_SB];
#pragma unroll
            for (int q = 0; q < HQ_SB; ++q) {
                const int e = min(e0 + 256 * q, total - 1);
                const int r = e / Q, c = e - r * Q;
                const int64_t b = b0 + r;
                sv[q] = *reinterpret_cast<const uint4*>(h16 + ((b < R ? b : R - 1) * Q + c) * 8);
            }
#pragma unroll
            for (int q = 0; q < HQ_SB; ++q) {
                const int e = e0 + 256 * q;
                if (e < total) {
                    const int r = e / Q, c = e - r * Q;
                    uint4 v = sv[q];
                    if (b0 + r >= R) v = make_uint4(0u, 0u, 0u, 0u);
                    *reinterpret_cast<uint4*>(hq_sm + (c & 1) * ROWS * LD + r * LD + (c >> 1) * 8) = v;
                }
            }
        }
    }
    __syncthreads();
    float best[NBT];
    int bidx[NBT];
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) { best[bt] = -INFINITY; bidx[bt] = 0x7FFFFFFF; }
    const int NCH = (KS + GEN_KC - 1) / GEN_KC;
    const int64_t first = t_lo + wave;
    const int64_t nt = first < t_hi ? (t_hi - first + 3) / 4 : 0;              // this wave's tiles: first, first + 4, ...
    const int64_t items = nt * NCH;                                            // (tile, chunk) pairs, in order
    f32x4 acc[NBT], acx[NBT];
    auto load_w = [&](int64_t it, f16x8 (&wf)[GEN_KC][2]) {
        const int64_t t = first + 4 * (it / NCH);
        const int c = (int)(it % NCH);
#pragma unroll
        for (int u = 0; u < GEN_KC; ++u) {
            const int ks = min(c * GEN_KC + u, KS - 1);                         // clamped: a duplicate k-step is not multiplied below
            const _Float16* wp = wfrag + ((t * KS + ks) * 2 * 64 + lane) * 8;
            wf[u][0] = *reinterpret_cast<const f16x8*>(wp);
            wf[u][1] = *reinterpret_cast<const f16x8*>(wp + 512);
        }
    };
    const _Float16* bp0 = hq_sm + c16 * LD + 8 * g4;
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
            if (ks < KS) {                                                     // wave-uniform
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
                const int64_t v = t * 16 + 4 * g4 + r;                         // ascending in r: '>' keeps the first index on ties
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
    // lanes l, l + 16, l + 32, l + 48 hold the same decode row: combine (first index wins ties)
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) {
#pragma unroll
        for (int sh = 16; sh <= 32; sh <<= 1) {
            const float ov = __shfl_xor(best[bt], sh);
            const int oi = __shfl_xor(bidx[bt], sh);
            if (ov > best[bt] || (ov == best[bt] && oi < bidx[bt])) { best[bt] = ov; bidx[bt] = oi; }
        }
    }
    // the four waves' winners meet in LDS (the staged rows are dead by now); one atomic max per workgroup and decode row, spread over the
    // row's ARGMAX_KEY_BUCKETS words (a key orders by value, then by the smaller index; a wave without a tile leaves the weakest key)
    unsigned long long* kl = reinterpret_cast<unsigned long long*>(hq_sm);      // [4 waves][ROWS]
    __syncthreads();
    if (g4 == 0) {
#pragma unroll
        for (int bt = 0; bt < NBT; ++bt) kl[wave * ROWS + bt * 16 + c16] = argmax_key(best[bt], bidx[bt]);
    }
    __syncthreads();
    if (tid < ROWS) {
        unsigned long long k = kl[tid];
#pragma unroll
        for (int w_ = 1; w_ < 4; ++w_) { const unsigned long long o = kl[w_ * ROWS + tid]; k = o > k ? o : k; }
        const int64_t b = b0 + tid;
        if (b < R && t_lo < t_hi) atomicMax(keys + b * ARGMAX_KEY_BUCKETS + (vr % ARGMAX_KEY_BUCKETS), k);
    }
}

// keys [nsteps][R][ARGMAX_KEY_BUCKETS] -> pred[row * pstride + step] (target-vocabulary ids); next (optional, nsteps = 1): next[row] =
// lut ? lut[pred] : pred, <unk> (1) outside [0, Vsrc)
__global__ void hq_keys_decode_kernel(const unsigned long long* __restrict__ keys, int64_t R, int nsteps, int64_t* __restrict__ pred, int64_t pstride,
                                      const int64_t* __restrict__ lut, int64_t Vsrc, int64_t* __restrict__ next) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= R * nsteps) return;
    const int64_t step = e / R, row = e - step * R;
    unsigned long long k = 0ull;
#pragma unroll
    for (int q = 0; q < ARGMAX_KEY_BUCKETS; ++q) { const unsigned long long o = keys[e * ARGMAX_KEY_BUCKETS + q]; k = o > k ? o : k; }
    const int64_t w = argmax_key_index(k);
    pred[row * pstride + step] = w;
    if (next) {
        const int64_t nxt = lut ? lut[w] : w;
        next[row] = (nxt >= 0 && nxt < Vsrc) ? nxt : 1;
    }
}

static int launch_hq_gen_argmax(const _Float16* h16, const void* frag, const float* bias, int64_t VT, int64_t R, int K, unsigned long long* keys,
                                hipStream_t st) {
    const int64_t ntiles = (VT + 15) / 16;
    const int nbt = gen_nbt(K);
    const int64_t nrb = (R + 16 * nbt - 1) / (16 * nbt);
    const int nvr = hq_nvr(nrb, ntiles);
    const size_t lds = gen_lds(K);
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute((const void*)hq_gen_argmax_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds(512));
        (void)hipFuncSetAttribute((const void*)hq_gen_argmax_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds(1024));
    });
    {
        ProfScope ps(prof_shape_name("hq_gen_argmax_kernel", (long long)R, (long long)VT, K), st);
        const dim3 grid((unsigned)(nvr * nrb));
        if (nbt == 4)
            hipLaunchKernelGGL(hq_gen_argmax_kernel<4>, grid, dim3(256), lds, st, h16, (const _Float16*)frag, bias, VT, ntiles, R, K, nvr, (int)nrb, keys);
        else
            hipLaunchKernelGGL(hq_gen_argmax_kernel<2>, grid, dim3(256), lds, st, h16, (const _Float16*)frag, bias, VT, ntiles, R, K, nvr, (int)nrb, keys);
    }
    NIR_CHECK_LAUNCH("hq_gen_argmax_kernel");
    return 0;
}

static int launch_hq_keys_decode(const unsigned long long* keys, int64_t R, int nsteps, int64_t* pred, int64_t pstride, const int64_t* lut,
                                 int64_t Vsrc, int64_t* next, hipStream_t st) {
    hipLaunchKernelGGL(hq_keys_decode_kernel, g1(R * nsteps), dim3(256), 0, st, keys, R, nsteps, pred, pstride, lut, Vsrc, next);
    NIR_CHECK_LAUNCH("hq_keys_decode_kernel");
    return 0;
}

struct HqPlan {
    float *h[2], *c[2], *h16[2], *logits;
    unsigned long long* keys;
    int64_t* tgt;
    size_t bytes;
};
static HqPlan hq_plan(void* ws, size_t cap, int64_t R, int H, int64_t VT, int max_len, bool fast) {
    Workspace a(ws, cap);
    HqPlan p;
    for (int k = 0; k < 2; ++k) { p.h[k] = a.take<float>((size_t)R * H); p.c[k] = a.take<float>((size_t)R * H); }
    for (int k = 0; k < 2; ++k) p.h16[k] = a.take<float>(fast ? (size_t)R * H : 0);      // the state as fp16 term pairs [R][H/8][2][8]
    p.logits = a.take<float>(fast ? 0 : (size_t)R * VT);
    p.keys = a.take<unsigned long long>(fast ? (size_t)max_len * R * ARGMAX_KEY_BUCKETS : 0);
    p.tgt = a.take<int64_t>((size_t)R);
    p.bytes = align_up(a.off, 256);
    return p;
}
}  // namespace nir

extern "C" size_t nir_hredqs_gen_argmax_workspace_bytes(int64_t rows) {
    if (rows <= 0) return 0;
    return (size_t)rows * nir::ARGMAX_KEY_BUCKETS * sizeof(unsigned long long) + 256;
}

extern "C" int nir_hredqs_gen_argmax(const void* h16, int64_t rows, int K, const float* gen_b, const void* gen_frag, int64_t VT,
                                     const int64_t* tgt2src, int64_t V, void* workspace, size_t workspace_bytes, int64_t* predictions,
                                     int64_t pred_stride, int64_t* next_tokens, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(h16 && gen_frag && predictions && next_tokens && workspace, "hredqs_gen_argmax: null pointer");
    NIR_REQUIRE(rows >= 0 && V > 0 && pred_stride >= 1, "hredqs_gen_argmax: bad dims");
    NIR_REQUIRE(gen_fusable(K, VT), "hredqs_gen_argmax: K must be a multiple of 32 in [32, 1024] and 0 < VT < 2^31 - 16");
    if (workspace_bytes < nir_hredqs_gen_argmax_workspace_bytes(rows)) {
        set_error("hredqs_gen_argmax: workspace too small");
        return NIR_ERR_WORKSPACE;
    }
    if (rows == 0) return 0;
    Workspace a(workspace, workspace_bytes);
    unsigned long long* keys = a.take<unsigned long long>((size_t)rows * ARGMAX_KEY_BUCKETS);
    NIR_PROPAGATE((int)hipMemsetAsync(keys, 0, (size_t)rows * ARGMAX_KEY_BUCKETS * sizeof(unsigned long long), st));
    NIR_PROPAGATE(launch_hq_gen_argmax((const _Float16*)h16, gen_frag, gen_b, VT, rows, K, keys, st));
    return launch_hq_keys_decode(keys, rows, 1, predictions, pred_stride, tgt2src, V, next_tokens, st);
}

extern "C" size_t nir_hredqs_decode_workspace_bytes(int64_t B, int64_t S, int max_len, const nir_hredqs_decoder_weights* w) {
    if (!nir::hq_weights_ok(w) || B < 0 || S < 0 || max_len < 0) return 0;
    return nir::hq_plan(nullptr, 0, B * S, w->H, w->VT, max_len, nir::hq_fast(w)).bytes;
}

extern "C" int nir_hredqs_decode_greedy(const float* h_steps, const float* c_steps, int64_t B, int64_t S, const float* table, int64_t V, int E,
                                        const int64_t* tgt2src, int64_t bos, int max_len, const nir_hredqs_decoder_weights* w, void* workspace,
                                        size_t workspace_bytes, int64_t* predictions, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(h_steps && c_steps && table && w && predictions, "hredqs_decode: null pointer");
    NIR_REQUIRE(hq_weights_ok(w), "hredqs_decode: decoder weights incomplete, H not a multiple of 4 or VT outside (0, 2^31 - 16)");
    NIR_REQUIRE(B >= 0 && S >= 0 && B * S < 0x7FFFFFFFLL && max_len >= 0 && V > 0 && E > 0 && E % 4 == 0, "hredqs_decode: bad dims");
    NIR_REQUIRE(bos >= 0 && bos < V, "hredqs_decode: BOS id outside the vocabulary");
    NIR_REQUIRE((w->rnn_gate_fold == nullptr) == (w->rnn_whh_frag == nullptr), "hredqs_decode: rnn_gate_fold and rnn_whh_frag come together");
    const int H = w->H;
    const int64_t R = B * S;
    const bool fast = hq_fast(w);
    HqPlan p = hq_plan(workspace, workspace_bytes, R, H, w->VT, max_len, fast);
    if (!workspace || p.bytes > workspace_bytes) {
        set_error("hredqs_decode: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
        return NIR_ERR_WORKSPACE;
    }
    if (R == 0 || max_len == 0) return 0;
    // the initial states in pairing order go where step 0 reads its previous state: slot 1 of the ping-pong buffers
    hipLaunchKernelGGL(hq_pair_kernel, g1(R * H), dim3(256), 0, st, h_steps, c_steps, B, S, H, p.h[1], p.c[1],
                       fast ? reinterpret_cast<_Float16*>(p.h16[1]) : nullptr);
    NIR_CHECK_LAUNCH("hq_pair_kernel");
    NIR_PROPAGATE(launch_fill_i64(p.tgt, bos, R, st));
    LstmStepArgs a = LstmStepArgs::token_fed(table, p.tgt, E, w->rnn_wih, w->rnn_whh, w->rnn_bih, w->rnn_bhh, R, H);
    if (fast) {
        a.fold_token_fed(w->rnn_gate_fold, w->rnn_whh_frag);
        NIR_PROPAGATE((int)hipMemsetAsync(p.keys, 0, (size_t)max_len * R * ARGMAX_KEY_BUCKETS * sizeof(unsigned long long), st));
    }
    for (int step = 0; step < max_len; ++step) {
        float* hn = p.h[step & 1];
        a.hprev[0] = p.h[(step + 1) & 1]; a.cprev[0] = p.c[(step + 1) & 1]; a.hnext[0] = hn; a.cnext[0] = p.c[step & 1];
        if (fast) {
            a.h16prev[0] = reinterpret_cast<const _Float16*>(p.h16[(step + 1) & 1]);
            a.h16next[0] = reinterpret_cast<_Float16*>(p.h16[step & 1]);
            if (step > 0) {                                  // the previous step's winner: key -> target id -> source id -> gate row, inside the step
                a.gxid[0] = nullptr; a.gxkey = p.keys + (size_t)(step - 1) * R * ARGMAX_KEY_BUCKETS; a.gxmap = tgt2src; a.gxV = V;
            }
            NIR_PROPAGATE(launch_lstm_step(a, 1, st));
            NIR_PROPAGATE(launch_hq_gen_argmax(a.h16next[0], w->gen_frag, w->gen_b, w->VT, R, H, p.keys + (size_t)step * R * ARGMAX_KEY_BUCKETS, st));
        } else {
            NIR_PROPAGATE(launch_lstm_step(a, 1, st));
            NIR_PROPAGATE(launch_linear(hn, H, nullptr, nullptr, 0, 0, 0, w->gen_w, H, w->gen_b, nullptr, p.logits, w->VT, R, (int)w->VT, H, NIR_ACT_NONE, st));
            NIR_PROPAGATE(launch_argmax_map(p.logits, w->VT, tgt2src, predictions + step, (int64_t)max_len, p.tgt, V, R, st));
        }
    }
    if (fast) NIR_PROPAGATE(launch_hq_keys_decode(p.keys, R, max_len, predictions, (int64_t)max_len, nullptr, 0, nullptr, st));
    return 0;
}
