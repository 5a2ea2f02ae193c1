// Seq2seq.decode -- greedy decoding of the attention encoder-decoder (neuroir/recommender/seq2seq.py:118-195; RNNDecoder:
// decoders/decoder.py:120-177, decoders/rnn_decoder.py:19-90; GlobalAttention 'general' / 'dot' / 'mlp': modules/global_attention.py:81-211).
//
// The step is written once, as the host-side S2sStepper (declared in s2s_gen.hpp, defined here): the argument checks, the two decisions (fused
// generator, fp16-term cell step), the shared part of the workspace plan, prepare() and step().  Three decodes are that stepper with a tail each:
// Seq2seq's greedy decode (arg-max) and ACG's (the copy generator of csrc/acg.hip) in s2s_decode below, the beam search in csrc/beam.hip.
//
// prepare(), once per decode: the bank the scores are taken against
//   general: memq = bank W_in     (score_j = (W_in h) . m_j = h . (W_in^T m_j): one GEMM instead of one per step)
//   dot:     memq = bank
//   mlp:     memc = bank W_c^T
// the BOS fill, the cell's arguments, and the initial state as fp16 term pairs when the fp16-term step runs.
// step(), for all decode rows at once (there is no input feed: the cell reads the previous token's embedding and its own state):
//   (h,c) = LSTM(emb(tok), (h,c))                     lstm_step_kernel (folded gate rows + fp16 term pairs, or the fp32 step);
//   h = GRU(emb(tok), h)                              the kernels of csrc/gru_step.hip
//   mlp only: qh = W_q h + b_q                        GEMM
//   a = softmax_j(mask(score_j)); ctx = sum_j a_j m_j; cat = [ctx ; h]; the attention row a                s2s_attend_kernel
//   o = linear_out(cat)  (+ tanh for general / dot; + bias, no tanh for mlp)                            GEMM + epilogue
// The greedy tail of Seq2seq:
//   tok' = argmax_v (W_g o + b_g)_v; tok = lut[tok']                                                    s2s_gen_argmax_kernel + argmax_finish_kernel
//                                                                                                    (or GEMM + argmax_map_kernel)
// Everything is enqueued on the caller's stream; no host synchronisation, no allocation, no float atomics.
#include <algorithm>
#include "s2s_gen.hpp"

namespace nir {

// ---- attention step: one wave per decode row -----------------------------------------------------------------------------------
// q: general / dot -- the decoder state h (the scores are h . sb_j); mlp -- W_q h + b_q (the scores are sum_f v_f tanh(q_f + sb[j, f])).
// sb [B, QL, H]: the score bank (memq / bank / memc);  mem [B, QL, H]: the memory bank the context is taken from.
// cat [B, 2H] = [ctx ; h];  attn row b at attn + b * attn_stride, [QL]: masked positions get an exact 0.0 (a row of length 0 is NaN
// throughout, like the reference's softmax over an all -inf row).
// nsrc: decode row i reads the banks and the length of source row i % nsrc (the greedy decoders pass nsrc = B; the beam of csrc/beam.hip
// has W decode rows per source row, row = k nsrc + b, and does not replicate the banks).
__global__ __launch_bounds__(256) void s2s_attend_kernel(const float* __restrict__ q, const float* __restrict__ h, const float* __restrict__ mem,
                                                         const float* __restrict__ sb, const float* __restrict__ v,
                                                         const int64_t* __restrict__ lens, int B, int QL, int H, int mlp, float* __restrict__ cat,
                                                         float* __restrict__ attn, int64_t attn_stride, int nsrc) {
    extern __shared__ float s2s_pr[];                 // [4][QL]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= B) return;
    float* pw = s2s_pr + wave * QL;
    const int si = i % nsrc;
    int len = (int)lens[si];
    len = len < 0 ? 0 : (len > QL ? QL : len);
    const float* mb = mem + (int64_t)si * QL * H;
    const float* sq = sb + (int64_t)si * QL * H;
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

// generator.weight [VT, K] fp32 -> the fragment order of s2s_gen.hpp (h1 rounded to nearest); err_flag bit 1: a weight outside the split's range
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

static int launch_gen_argmax(const float* x, const void* frag, const float* bias, int64_t VT, int64_t Bd, int K, float* pval, int* pidx,
                             const int64_t* lut, int64_t* pred, int64_t pstride, int64_t* tgt, int64_t Vsrc, hipStream_t st) {
    int nparts;
    NIR_PROPAGATE(launch_gen_argmax_partials<false>("s2s_gen_argmax_kernel", x, frag, bias, VT, Bd, K, pval, pidx, nullptr, &nparts, st));
    return launch_argmax_finish(pval, pidx, nparts, Bd, lut, pred, pstride, tgt, Vsrc, st);
}

int launch_attend(const float* q, const float* h, const float* mem, const float* sb, const float* v, const int64_t* lens, int64_t B, int QL, int H,
                  int mlp, float* cat, float* attn, int64_t attn_stride, hipStream_t st, int64_t nsrc) {
    {
        ProfScope ps("s2s_attend_kernel", st);
        hipLaunchKernelGGL(s2s_attend_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), (size_t)4 * QL * sizeof(float), st, q, h, mem, sb, v, lens, (int)B,
                           QL, H, mlp, cat, attn, attn_stride, (int)(nsrc > 0 ? nsrc : B));
    }
    NIR_CHECK_LAUNCH("s2s_attend_kernel");
    return 0;
}

S2sStepBufs s2s_step_bufs(Workspace& a, int64_t rows, int64_t nsrc, int QL, int H, int64_t VT, int attn_type, bool fused, int cell, bool h16) {
    S2sStepBufs b;
    b.sb = a.take<float>(attn_type == NIR_S2S_ATTN_DOT ? 0 : (size_t)nsrc * QL * H);
    for (int k = 0; k < 2; ++k) { b.h[k] = a.take<float>((size_t)rows * H); b.c[k] = a.take<float>(cell == S2S_CELL_GRU ? 0 : (size_t)rows * H); }
    for (int k = 0; k < 2; ++k) b.h16[k] = a.take<float>(h16 ? (size_t)rows * H : 0);
    b.qh = a.take<float>(attn_type == NIR_S2S_ATTN_MLP ? (size_t)rows * H : 0);
    b.cat = a.take<float>((size_t)rows * 2 * H);
    b.ah = a.take<float>((size_t)rows * H);
    b.logits = a.take<float>(fused ? 0 : (size_t)rows * VT);
    b.tgt = nullptr;
    b.gru = nullptr;
    return b;
}

struct S2sPlan {
    S2sStepBufs s;
    float* pval;
    int* pidx;
    float* psum;                                      // ACG only: the sums of the partials
    AcgCopyAttn ca;                                   // ACG only: a copy attention of its own
    size_t bytes;
};
// acg: 0 = Seq2seq, 1 = ACG with reuse_copy_attn, 2 = ACG with a copy attention of its own
static S2sPlan s2s_plan(void* ws, size_t cap, int64_t B, int QL, int H, int64_t VT, int attn_type, bool fused, int acg = 0, int cell = S2S_CELL_LSTM) {
    Workspace a(ws, cap);
    S2sPlan p;
    p.s = s2s_step_bufs(a, B, B, QL, H, VT, attn_type, fused, cell, true);
    p.pval = a.take<float>(fused ? (size_t)S2S_MAX_WGS * 4 * B : 0);
    p.pidx = a.take<int>(fused ? (size_t)S2S_MAX_WGS * 4 * B : 0);
    p.s.tgt = a.take<int64_t>((size_t)B);
    p.psum = nullptr;
    if (acg) {
        if (!fused) { p.pval = a.take<float>((size_t)B); p.pidx = a.take<int>((size_t)B); }      // one partial per row behind the GEMM
        p.psum = a.take<float>(fused ? (size_t)S2S_MAX_WGS * 4 * B : (size_t)B);
    }
    if (acg == 2) p.ca.carve(a, B, B, QL, H, attn_type);
    if (cell == S2S_CELL_GRU) p.s.gru = a.take<float>(gru_step_scratch_floats(B, H));
    p.bytes = align_up(a.off, 256);
    return p;
}
bool s2s_fused(const nir_seq2seq_decoder_weights* w) { return s2s_gen_fused(w->gen_frag, w->H, w->VT); }
bool s2s_step16(const nir_seq2seq_decoder_weights* w) { return w->rnn_gate_fold && w->rnn_whh_frag && w->H % 32 == 0 && !tun(g_tun.exact_f32); }
bool s2s_weights_ok(const nir_seq2seq_decoder_weights* w) {
    if (!w || w->H <= 0 || w->H % 4 || w->VT <= 0) return false;
    if (!(w->rnn_wih && w->rnn_whh && w->rnn_bih && w->rnn_bhh && w->attn_out_w && w->gen_w && w->gen_b)) return false;
    if (w->attn_type == NIR_S2S_ATTN_GENERAL) return w->attn_in_wt != nullptr;
    if (w->attn_type == NIR_S2S_ATTN_DOT) return true;
    if (w->attn_type == NIR_S2S_ATTN_MLP) return w->attn_ctx_w && w->attn_query_w && w->attn_query_b && w->attn_v && w->attn_out_b;
    return false;
}

int S2sStepper::check(const float* dec_h, const float* dec_c, bool outputs, int64_t bos, int max_len) {
    NIR_REQUIRE(dec_h && (dec_c || cell == S2S_CELL_GRU) && memory_bank && source_len && table && w && outputs, "%s: null pointer", name);
    NIR_REQUIRE(s2s_weights_ok(w), "%s: decoder weights incomplete for the attention type, or H not a multiple of 4", name);
    NIR_REQUIRE(nsrc >= 0 && QL > 0 && QL <= 4096 && max_len > 0 && V > 0 && E > 0 && E % 4 == 0, "%s: bad dims", name);
    NIR_REQUIRE(bos >= 0 && bos < V, "%s: BOS id outside the vocabulary", name);
    NIR_REQUIRE((w->rnn_gate_fold == nullptr) == (w->rnn_whh_frag == nullptr), "%s: rnn_gate_fold and rnn_whh_frag come together", name);
    fused = s2s_fused(w);
    NIR_REQUIRE(fused || w->VT < 0x7FFFFFFFLL, "%s: VT too large for the GEMM path", name);
    step16 = s2s_step16(w);
    return 0;
}

int S2sStepper::prepare(const float* dec_h, int64_t bos, float* h16first) {
    const int H = w->H;
    sb = memory_bank;
    if (w->attn_type != NIR_S2S_ATTN_DOT) {              // general: memq = bank W_in (global_attention.py:98-105); mlp: memc = linear_context(bank) (:112-114)
        NIR_PROPAGATE(launch_linear(memory_bank, H, nullptr, nullptr, 0, 0, 0, w->attn_type == NIR_S2S_ATTN_MLP ? w->attn_ctx_w : w->attn_in_wt, H, nullptr,
                                    nullptr, b.sb, H, nsrc * QL, H, H, NIR_ACT_NONE, st));
        sb = b.sb;
    }
    NIR_PROPAGATE(launch_fill_i64(b.tgt, bos, rows, st));
    if (cell == S2S_CELL_GRU) {
        ga.tok = b.tgt; ga.V = V; ga.table = table; ga.E = E;
        ga.wih = w->rnn_wih; ga.bih = w->rnn_bih; ga.whh = w->rnn_whh; ga.bhh = w->rnn_bhh;
        ga.scratch = b.gru; ga.B = rows; ga.H = H;
        if (step16) { ga.gate_fold = w->rnn_gate_fold; ga.whh_frag = w->rnn_whh_frag; }
    } else {
        a = LstmStepArgs::token_fed(table, b.tgt, E, w->rnn_wih, w->rnn_whh, w->rnn_bih, w->rnn_bhh, rows, H);
        if (step16) a.fold_token_fed(w->rnn_gate_fold, w->rnn_whh_frag);
    }
    if (step16) NIR_PROPAGATE(launch_h16_pack(dec_h, rows * H, reinterpret_cast<_Float16*>(h16first), st));
    return 0;
}

int S2sStepper::step(const float* hp, const float* cp, float* hn, float* cn, const float* h16prev, float* h16next, float* attn_out, int64_t attn_stride) {
    const int H = w->H;
    const bool mlp = w->attn_type == NIR_S2S_ATTN_MLP;
    if (step16) {
        a.h16prev[0] = ga.h16prev = reinterpret_cast<const _Float16*>(h16prev);
        a.h16next[0] = ga.h16next = reinterpret_cast<_Float16*>(h16next);
    }
    if (cell == S2S_CELL_GRU) {
        ga.hprev = hp; ga.hnext = hn;
        NIR_PROPAGATE(launch_gru_step(ga, st));
    } else {
        a.hprev[0] = hp; a.cprev[0] = cp; a.hnext[0] = hn; a.cnext[0] = cn;
        NIR_PROPAGATE(launch_lstm_step(a, 1, st));
    }
    if (mlp)
        NIR_PROPAGATE(launch_linear(hn, H, nullptr, nullptr, 0, 0, 0, w->attn_query_w, H, w->attn_query_b, nullptr, b.qh, H, rows, H, H, NIR_ACT_NONE, st));
    NIR_PROPAGATE(launch_attend(mlp ? b.qh : hn, hn, memory_bank, sb, w->attn_v, source_len, rows, QL, H, mlp, b.cat, attn_out, attn_stride, st, nsrc));
    return launch_linear(b.cat, 2 * H, nullptr, nullptr, 0, 0, 0, w->attn_out_w, 2 * H, mlp ? w->attn_out_b : nullptr, nullptr, b.ah, H, rows, H, 2 * H,
                         mlp ? NIR_ACT_NONE : NIR_ACT_TANH, st);
}

bool acg_weights_ok(const nir_seq2seq_decoder_weights* w, const AcgDecode* g) {
    if (!g->cw || !g->cw->copy_w || !g->cw->copy_b) return false;
    if (g->cw->reuse_copy_attn) return true;
    if (w->attn_type == NIR_S2S_ATTN_GENERAL) return g->cw->attn_in_wt != nullptr;
    if (w->attn_type == NIR_S2S_ATTN_MLP) return g->cw->attn_ctx_w && g->cw->attn_query_w && g->cw->attn_query_b && g->cw->attn_v;
    return true;
}

size_t s2s_decode_workspace_bytes(int64_t B, int QL, const nir_seq2seq_decoder_weights* w, const AcgDecode* acg, int cell) {
    if (!s2s_weights_ok(w) || B < 0 || QL <= 0 || (acg && !acg_weights_ok(w, acg))) return 0;
    return s2s_plan(nullptr, 0, B, QL, w->H, w->VT, w->attn_type, s2s_fused(w), acg ? (acg->cw->reuse_copy_attn ? 1 : 2) : 0, cell).bytes;
}

}  // namespace nir

extern "C" size_t nir_seq2seq_gen_frag_bytes(int64_t VT, int K) {
    if (!nir::gen_fusable(K, VT)) return 0;
    return (size_t)((VT + 15) / 16) * (K / 32) * 2 * 64 * 8 * sizeof(_Float16);
}

extern "C" int nir_seq2seq_pack_gen_frag(const float* gen_w, int64_t VT, int K, void* frag, int* err_flag, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(gen_w && frag, "seq2seq_pack_gen_frag: null pointer");
    NIR_REQUIRE(gen_fusable(K, VT), "seq2seq_pack_gen_frag: K must be a multiple of 32 in [32, 1024] and 0 < VT < 2^31 - 16");
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
    const bool fused = s2s_gen_fused(gen_frag, K, VT);
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
    return nir::s2s_decode_workspace_bytes(B, QL, w, nullptr, nir::S2S_CELL_LSTM);
}

extern "C" int nir_seq2seq_decode_greedy(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B,
                                         int QL, const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                                         const nir_seq2seq_decoder_weights* w, void* workspace, size_t workspace_bytes, int64_t* predictions,
                                         float* attentions, nir_stream_t stream) {
    return nir::s2s_decode(dec_h, dec_c, memory_bank, source_len, B, QL, table, V, E, tgt2src, bos, max_len, w, workspace, workspace_bytes, predictions,
                           attentions, nullptr, nir::S2S_CELL_LSTM, (hipStream_t)stream);
}

// The same decode with a GRU decoder (decoders/decoder.py:175-177, decoders/rnn_decoder.py:46-47): no cell state; rnn_* are [3H, .], rnn_gate_fold
// and rnn_whh_frag the GRU forms (csrc/gru_step.hip).
extern "C" size_t nir_seq2seq_gru_decode_workspace_bytes(int64_t B, int QL, const nir_seq2seq_decoder_weights* w) {
    return nir::s2s_decode_workspace_bytes(B, QL, w, nullptr, nir::S2S_CELL_GRU);
}

extern "C" int nir_seq2seq_gru_decode_greedy(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL,
                                             const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                                             const nir_seq2seq_decoder_weights* w, void* workspace, size_t workspace_bytes, int64_t* predictions,
                                             float* attentions, nir_stream_t stream) {
    return nir::s2s_decode(dec_h, nullptr, memory_bank, source_len, B, QL, table, V, E, tgt2src, bos, max_len, w, workspace, workspace_bytes, predictions,
                           attentions, nullptr, nir::S2S_CELL_GRU, (hipStream_t)stream);
}

// The greedy decode of both attention recommenders: the stepper (s2s_gen.hpp) with one of two tails behind the attentional output.  acg == NULL is
// Seq2seq's (generator + arg-max); otherwise ACG's, the copy generator of csrc/acg.hip -- and, without reuse_copy_attn, a second attention on the
// attentional output in front of it.  The state ping-pongs: step s writes slot s & 1 and reads the other.
int nir::s2s_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, const float* table,
                    int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w, void* workspace,
                    size_t workspace_bytes, int64_t* predictions, float* attentions, const AcgDecode* acg, int cell, hipStream_t st) {
    S2sStepper s{"seq2seq_decode", w, cell, table, memory_bank, source_len, V, B, B, E, QL, st};
    NIR_PROPAGATE(s.check(dec_h, dec_c, predictions && attentions, bos, max_len));
    const int H = w->H;
    const bool fused = s.fused;
    if (acg) {
        NIR_REQUIRE(acg_weights_ok(w, acg), "acg_decode: copy weights incomplete for the attention type");
        NIR_REQUIRE(acg->src_map_idx && acg->ext2tgt && acg->ext2src, "acg_decode: null index tensor");
        NIR_REQUIRE(acg_dims_ok(QL, acg->CV), "acg_decode: CV outside [2, %d]", ACG_MAX_CV);
    }
    S2sPlan p = s2s_plan(workspace, workspace_bytes, B, QL, H, w->VT, w->attn_type, fused, acg ? (acg->cw->reuse_copy_attn ? 1 : 2) : 0, cell);
    if (!workspace || p.bytes > workspace_bytes) {
        set_error("seq2seq_decode: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
        return NIR_ERR_WORKSPACE;
    }
    if (B == 0) return 0;
    s.b = p.s;
    NIR_PROPAGATE(s.prepare(dec_h, bos, p.s.h16[1]));
    if (acg) NIR_PROPAGATE(p.ca.prepare(acg->cw, memory_bank, B, QL, H, w->attn_type, st));
    const float* hp = dec_h;
    const float* cp = dec_c;
    for (int step = 0; step < max_len; ++step) {
        float* hn = p.s.h[step & 1];
        float* cn = p.s.c[step & 1];
        NIR_PROPAGATE(s.step(hp, cp, hn, cn, p.s.h16[(step + 1) & 1], p.s.h16[step & 1], attentions + (int64_t)step * QL, (int64_t)max_len * QL));
        const float* ah = p.s.ah;
        if (acg) {
            const float* ca = attentions + (int64_t)step * QL;                 // the copy attention: the std one, or ACG's own
            int64_t ca_stride = (int64_t)max_len * QL;
            NIR_PROPAGATE(p.ca.step(acg->cw, ah, B, B, memory_bank, source_len, QL, H, w->attn_type, &ca, &ca_stride, st));
            NIR_PROPAGATE(launch_acg_gen_select(ah, B, H, w->gen_w, w->gen_b, fused ? w->gen_frag : nullptr, w->VT, p.s.logits, p.pval, p.pidx, p.psum,
                                                acg->cw->copy_w, acg->cw->copy_b, ca, ca_stride, source_len, QL, acg->src_map_idx, acg->ext2tgt,
                                                acg->ext2src, acg->CV, tgt2src, V, predictions + step, (int64_t)max_len, p.s.tgt, st));
        } else if (fused) {
            NIR_PROPAGATE(launch_gen_argmax(ah, w->gen_frag, w->gen_b, w->VT, B, H, p.pval, p.pidx, tgt2src, predictions + step, (int64_t)max_len, p.s.tgt, V,
                                            st));
        } else {
            NIR_PROPAGATE(launch_linear(ah, H, nullptr, nullptr, 0, 0, 0, w->gen_w, H, w->gen_b, nullptr, p.s.logits, w->VT, B, (int)w->VT, H, NIR_ACT_NONE, st));
            NIR_PROPAGATE(launch_argmax_map(p.s.logits, w->VT, tgt2src, predictions + step, (int64_t)max_len, p.s.tgt, V, B, st));
        }
        hp = hn;
        cp = cn;
    }
    return 0;
}
