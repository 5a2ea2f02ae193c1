// Shared by the decoders (csrc/cars_decode.hip, csrc/seq2seq.hip, csrc/hredqs.hip, csrc/beam.hip): the GEMM launchers of gemm.hip and the small
// launches every decoder makes between its steps.  The kernels live in cars_decode.hip; these are their host-side launchers.
#pragma once
#include <algorithm>
#include "split2.hpp"

namespace nir {

int launch_linear(const float* a, int64_t lda, const int64_t* ids, const float* table, int E, int64_t rows_per_seq,
                  int64_t seq_stride, const float* w, int64_t ldw, const float* bias, const float* bias2, float* c,
                  int64_t ldc, int64_t M, int N, int K, int act, hipStream_t st);

int launch_linear_ex(const float* a, int64_t lda, const int64_t* ids, const float* table, int E, int64_t rows_per_seq,
                     int64_t seq_stride, const float* w, int64_t ldw, const float* bias, const float* bias2, float* c,
                     int64_t ldc, int64_t M, int N, int K, int act, const float* add, int64_t ldadd, hipStream_t st);
// The CARS decoder's attention (csrc/cars_decode.hip: dec_attend_kernel) over `rows` decode rows: row i scores qv[i] against memq[rowmap[i]], pools
// mem[rowmap[i]] over the first lens[rowmap[i]] positions and writes cat[i] = [ctx ; h[i]]
int launch_dec_attend(const float* qv, const float* h, const float* mem, const float* memq, const int64_t* rowmap, const int64_t* lens, int64_t rows, int QL,
                      int HD, float* cat, hipStream_t st);
// p[i] = v, i < n
int launch_fill_i64(int64_t* p, int64_t v, int64_t n, hipStream_t st);
// h [n = rows * H] fp32 -> the fp16 term pairs of the fp16-term LSTM step: [row][H/8][2 terms][8]  (H % 8 == 0)
int launch_h16_pack(const float* h, int64_t n, _Float16* out, hipStream_t st);
// pred[i * pstride] = argmax_v logits[i, v] (first index on ties); tgt[i] = lut ? lut[pred] : pred, <unk> (1) outside [0, Vsrc)
int launch_argmax_map(const float* logits, int64_t V, const int64_t* lut, int64_t* pred, int64_t pstride, int64_t* tgt, int64_t Vsrc, int64_t Bd,
                      hipStream_t st);
// the same from `nparts` partial (value, index) pairs per row, pval / pidx [nparts][Bd]
int launch_argmax_finish(const float* pval, const int* pidx, int nparts, int64_t Bd, const int64_t* lut, int64_t* pred, int64_t pstride, int64_t* tgt,
                         int64_t Vsrc, hipStream_t st);
// multiProcessorCount of the current device (256 if unknown)
int device_cu_count();

// ---- the launch geometry of the fused generator kernels (s2s_gen.hpp: s2s_gen_argmax_kernel; csrc/hredqs.hip: hq_gen_argmax_kernel;
// csrc/beam.hip: beam_gen_topk_kernel) and the form test of the HredQS decode entries ---------------------------------------------------------
constexpr int GEN_KC = 8;                             // k-steps a chunk
constexpr int S2S_MAX_WGS = 256;

static inline int gen_nbt(int K) { return K <= 512 ? 4 : 2; }
static inline size_t gen_lds(int K) { return (size_t)2 * 16 * gen_nbt(K) * (K + 8) * sizeof(_Float16); }
static inline bool gen_fusable(int K, int64_t VT) { return K >= 32 && K <= 1024 && K % 32 == 0 && VT > 0 && VT < 0x7FFFFFF0LL; }

// vocabulary ranges of the kernels on fp32 rows (s2s_gen_argmax_kernel, beam_gen_topk_kernel on BeamRowsF32): workgroups per row block, enough for the chip, at least ~2 tiles per wave
static inline int s2s_nvr(int64_t Bd, int K, int64_t ntiles) {
    const int64_t rb = (Bd + 16 * gen_nbt(K) - 1) / (16 * gen_nbt(K));
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(S2S_MAX_WGS, (device_cu_count() + rb - 1) / rb), (ntiles + 7) / 8));
}
// vocabulary ranges of the kernels on the split state (hq_gen_argmax_kernel, beam_gen_topk_kernel on BeamRowsSplit): one workgroup per CU
// (the staged rows fill its LDS) in a single round, at least ~2 tiles per wave; a multiple of 8 from 8 on, so that the row blocks of a
// range can share an XCD
static inline int hq_nvr(int64_t nrb, int64_t ntiles) {
    int64_t n = std::max<int64_t>(1, std::min<int64_t>(device_cu_count() / nrb, (ntiles + 7) / 8));
    if (n >= 8) n -= n % 8;
    return (int)n;
}

static inline bool hq_weights_ok(const nir_hredqs_decoder_weights* w) {
    return w && w->H > 0 && w->H % 4 == 0 && w->VT > 0 && w->VT < 0x7FFFFFF0LL && w->rnn_wih && w->rnn_whh && w->rnn_bih && w->rnn_bhh && w->gen_w &&
           w->gen_b;
}
static inline bool hq_fast(const nir_hredqs_decoder_weights* w) {
    return w->rnn_gate_fold && w->rnn_whh_frag && w->gen_frag && gen_fusable(w->H, w->VT) && !tun(g_tun.exact_f32);
}

// One GRU decoder step (csrc/gru_step.hip).  Fast form (gru_step_fast): whh_frag, h16prev and h16next given, H % 32 == 0, tunable exact_f32 off --
// one launch when gate_fold is given too, else the gathered input GEMM into `scratch` in front of it.  Plain form otherwise: exact fp32, three
// launches through `scratch` (gru_step_scratch_floats), h16next filled behind them when given.  hnext must not alias hprev.
struct GruStepArgs {
    const int64_t* tok = nullptr;         // [B] token ids, already inside [0, V) (the fast form clamps what it gathers the table by all the same)
    int64_t V = 0;
    const float* gate_fold = nullptr;     // [V,3H] = table W_ih^T + b_ih + (b_hr, b_hz, 0), or NULL
    const float* table = nullptr;         // [V,E] with wih [3H,E], bih [3H]: read when gate_fold is NULL or the plain form runs
    int E = 0;
    const float *wih = nullptr, *bih = nullptr;
    const float *whh = nullptr, *bhh = nullptr;      // [3H,H], [3H]
    const void* whh_frag = nullptr;       // nir_gru_step_pack_whh_frag(whh, H)
    const float* hprev = nullptr;         // [B,H]
    const _Float16* h16prev = nullptr;    // [B][H/8][2 terms][8]
    float* hnext = nullptr;
    _Float16* h16next = nullptr;
    float* scratch = nullptr;
    int64_t B = 0;
    int H = 0;
};
bool gru_step_fast(const GruStepArgs& a);
size_t gru_step_scratch_floats(int64_t B, int H);
int launch_gru_step(const GruStepArgs& a, hipStream_t st);

}  // namespace nir
