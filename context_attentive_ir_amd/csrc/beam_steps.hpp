// The step helpers the beam decodes (csrc/beam.hip) share with the sampling decodes of the session models and HredQS (csrc/session_sample.hip):
// both walk R = Bd W (or Bd N) un-repeated rows, row r reading what decode row r % Bd reads.  The kernels live in csrc/beam.hip.
#pragma once
#include "s2s_gen.hpp"

namespace nir {

// the first state of every beam row (and the repeated row map) into slot 0; h16first given: and its fp16 term pairs, for the fp16-term step
int launch_beam_repeat(const float* dec_h, const float* dec_c, int64_t Bd, int64_t R, int H, float* h0, float* c0, float* h16first,
                       const int64_t* map_in, int64_t* map_out, hipStream_t st);
// HredQS: pairing, repeat and split in one launch (hq_beam_begin_kernel) -- row k Bd + i takes the state of step i / B of session i % B
int launch_hq_beam_begin(const float* hs, const float* cs, int64_t B, int64_t S, int H, int64_t R, float* h0, float* c0, _Float16* h16, hipStream_t st);

// the token-fed LSTM step of these decoders over the R beam rows, every step from state slot 0 (the reordered one) into slot 1; step16: the
// fp16-term step on gate_fold and whh_frag, with the states' term pairs h16
static inline LstmStepArgs beam_lstm_step_args(const float* table, const int64_t* tgt, int E, const float* w_ih, const float* w_hh, const float* b_ih,
                                        const float* b_hh, bool step16, const float* gate_fold, const void* whh_frag, int64_t R, int H, float* const* h,
                                        float* const* c, float* const* h16) {
    LstmStepArgs a = LstmStepArgs::token_fed(table, tgt, E, w_ih, w_hh, b_ih, b_hh, R, H);
    a.hprev[0] = h[0]; a.cprev[0] = c[0]; a.hnext[0] = h[1]; a.cnext[0] = c[1];
    if (step16) {
        a.fold_token_fed(gate_fold, whh_frag);
        a.h16prev[0] = reinterpret_cast<const _Float16*>(h16[0]);
        a.h16next[0] = reinterpret_cast<_Float16*>(h16[1]);
    }
    return a;
}

// nir_acg_beam_gen_select for the sampler's top-k form (csrc/sample.hip).  logit_targets: in the plain form a collapse target's logit is read from
// the GEMM's workspace logits (what m and Z were formed from) instead of the wave's row dot; the beam's own entry passes false
int acg_beam_gen_select_rows(const float* o, int64_t rows, int64_t nsrc, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                             int W, const float* copy_w, const float* copy_b, const float* copy_attn, int64_t attn_stride, const int64_t* source_len, int QL,
                             const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src, int CV, void* workspace, size_t workspace_bytes,
                             float* top_val, int32_t* top_idx, nir_stream_t stream, bool logit_targets);

static inline bool cars_beam_step16(const nir_cars_decoder_weights* w) { return w->rnn_gate_fold && w->rnn_whh_frag && w->HD % 32 == 0 && !tun(g_tun.exact_f32); }
static inline bool cars_beam_weights_ok(const nir_cars_decoder_weights* w) {
    return w && w->rnn_wih && w->rnn_whh && w->rnn_bih && w->rnn_bhh && w->attn_out_w && w->dec_attn_w && w->pred1_w && w->pred2_w &&
           (w->attn_in_w || w->attn_q_w) && w->HD > 0 && w->DQ > 0 && w->P > 0 && w->KS >= 0 && w->VT > 0 && w->HD % 4 == 0 && w->DQ % 4 == 0 && w->P % 4 == 0;
}

}  // namespace nir
