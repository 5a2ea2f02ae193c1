// The step helpers the beam decodes (csrc/beam.hip) share with the sampling decodes of the session models and HredQS (csrc/session_sample.hip):
// both walk R = Bd W (or Bd N) un-repeated rows, row r reading what decode row r % Bd reads.  The kernels live in csrc/beam.hip.  The CARS
// decoder's whole step over those rows is written here once (CarsRowsStep): the two decodes differ in the state slots they read and write.
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

// ---- the CARS decoder step over R un-repeated rows, once ------------------------------------------------------------------------------------------
// The step of nir_cars_decode_greedy restated over R rows (its keyed arg-max path ties the greedy loop's launches to its own tail; the greedy
// entry stays as it is), for the beam (csrc/beam.hip: R = Bd W, every step from state slot 0 into slot 1) and the sampling decode
// (csrc/session_sample.hip: R = Bd N, the slots ping-pong).  prepare once -- the banks mem / memq over the source rows, the first state of every
// row into a given slot, the session projection over the R rows through the repeated rowmap -- then per step lstm step, (linear_in,) dec_attend,
// linear_out + tanh, pred1 + session term: behind step() p1 [R, P] is what the generator reads.
struct CarsRowsStep {
    float *mem, *memq, *sess, *h[2], *c[2], *h16[2], *qv, *cat, *ah, *p1;
    int64_t* rowmap;
    const nir_cars_decoder_weights* w;                // set by carve()
    int64_t R;
    int QL;
    bool foldq, step16;
    const int64_t* source_len;                        // set by prepare()
    LstmStepArgs a;
    hipStream_t st;
    // takes mem .. rowmap, in this order
    void carve(Workspace& ws, int64_t rows_src, int64_t R_, int QL_, const nir_cars_decoder_weights* w_) {
        w = w_, R = R_, QL = QL_, foldq = w->attn_q_w != nullptr, step16 = cars_beam_step16(w);
        const int HD = w->HD, P = w->P;
        mem = ws.take<float>((size_t)rows_src * QL * HD);
        memq = ws.take<float>(foldq ? (size_t)rows_src * QL * HD : 0);
        sess = ws.take<float>(w->KS > 0 ? (size_t)R * P : 0);
        for (int k = 0; k < 2; ++k) { h[k] = ws.take<float>((size_t)R * HD); c[k] = ws.take<float>((size_t)R * HD); }
        for (int k = 0; k < 2; ++k) h16[k] = ws.take<float>(step16 ? (size_t)R * HD : 0);
        qv = ws.take<float>(foldq ? 0 : (size_t)R * HD);
        cat = ws.take<float>((size_t)R * 2 * HD);
        ah = ws.take<float>((size_t)R * HD);
        p1 = ws.take<float>((size_t)R * P);
        rowmap = ws.take<int64_t>((size_t)R);
    }
    // once per decode, as the greedy entry: the banks over every source row, the first state into `slot`, tail_begin() -- the tail's own first
    // launches, which fill tgt --, the session projection (gathered through the repeated rowmap), the cell's arguments
    template <class TailBegin>
    int prepare(const float* dec_h, const float* dec_c, const float* encoded_source, const int64_t* source_len_, int64_t rows_src, const int64_t* rowmap_in,
                int64_t Bd, const float* session_cat, const float* table, const int64_t* tgt, int E, int slot, hipStream_t st_, TailBegin tail_begin) {
        const int HD = w->HD, P = w->P;
        source_len = source_len_, st = st_;
        NIR_PROPAGATE(launch_linear(encoded_source, w->DQ, nullptr, nullptr, 0, 0, 0, w->dec_attn_w, w->DQ, nullptr, nullptr, mem, HD, rows_src * QL, HD, w->DQ,
                                    NIR_ACT_NONE, st));
        if (foldq)
            NIR_PROPAGATE(launch_linear(encoded_source, w->DQ, nullptr, nullptr, 0, 0, 0, w->attn_q_w, w->DQ, nullptr, nullptr, memq, HD, rows_src * QL, HD, w->DQ,
                                        NIR_ACT_NONE, st));
        NIR_PROPAGATE(launch_beam_repeat(dec_h, dec_c, Bd, R, HD, h[slot], c[slot], step16 ? h16[slot] : nullptr, rowmap_in, rowmap, st));
        NIR_PROPAGATE(tail_begin());
        if (w->KS > 0)
            NIR_PROPAGATE(launch_linear(nullptr, 0, rowmap, session_cat, w->KS, 1, 1, w->sess_w, w->KS, nullptr, nullptr, sess, P, R, P, w->KS, NIR_ACT_NONE, st));
        a = beam_lstm_step_args(table, tgt, E, w->rnn_wih, w->rnn_whh, w->rnn_bih, w->rnn_bhh, step16, w->rnn_gate_fold, w->rnn_whh_frag, R, HD, h, c, h16);
        return 0;
    }
    // one step from state slot rd into slot wr
    int step(int rd, int wr) {
        const int HD = w->HD, P = w->P;
        float* hn = h[wr];
        a.hprev[0] = h[rd]; a.cprev[0] = c[rd]; a.hnext[0] = hn; a.cnext[0] = c[wr];
        if (step16) {
            a.h16prev[0] = reinterpret_cast<const _Float16*>(h16[rd]);
            a.h16next[0] = reinterpret_cast<_Float16*>(h16[wr]);
        }
        NIR_PROPAGATE(launch_lstm_step(a, 1, st));
        if (!foldq) NIR_PROPAGATE(launch_linear(hn, HD, nullptr, nullptr, 0, 0, 0, w->attn_in_w, HD, nullptr, nullptr, qv, HD, R, HD, HD, NIR_ACT_NONE, st));
        NIR_PROPAGATE(launch_dec_attend(foldq ? hn : qv, hn, mem, foldq ? memq : mem, rowmap, source_len, R, QL, HD, cat, st));
        NIR_PROPAGATE(launch_linear(cat, 2 * HD, nullptr, nullptr, 0, 0, 0, w->attn_out_w, 2 * HD, nullptr, nullptr, ah, HD, R, HD, 2 * HD, NIR_ACT_TANH, st));
        return launch_linear_ex(ah, HD, nullptr, nullptr, 0, 0, 0, w->pred1_w, HD, nullptr, nullptr, p1, P, R, P, HD, NIR_ACT_NONE, w->KS > 0 ? sess : nullptr, P,
                                st);
    }
};

}  // namespace nir
