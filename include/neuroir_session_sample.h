/* libneuroir_hip: sampling decode for HredQS and the session models (CARS, M_MATCH_TENSOR, MNSRF).  Included by neuroir_hip.h (which defines
 * the types used here); not meant to be included on its own.  csrc/session_sample.hip, csrc/sample.hip; DESIGN.md section 29. */
#ifndef NEUROIR_SESSION_SAMPLE_H
#define NEUROIR_SESSION_SAMPLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * The draw is the one of neuroir_sample.h -- noise, choice, top_k, logp, freeze, feedback, horizon, the PAD caveat: read its head -- with
 * "source row" read as "decode row of the greedy decode", the reading neuroir_session_beam.h and neuroir_hredqs_beam.h make for the search.
 *   rows      Bd decode rows (session models: B (S-1); HredQS: B S in (b, s) order), N >= 1 samples each: R = Bd N sample rows, row r = n Bd + i.
 *             The noise is keyed by (seed, step, i, n, v): nsrc = Bd.
 *   inputs    nothing is repeated by the caller: sample row r reads what decode row r % Bd reads (CARS: rowmap, encoded_source, source_len,
 *             session_cat, as in nir_beam_cars_decode).  HredQS pairs the states itself, as nir_beam_hredqs_decode does: decode row i starts
 *             from step i / B of session i % B.
 *   outputs   in sample order: predictions [Bd, N, max_len] int64, token_logprobs [Bd, N, max_len] fp32, scores [Bd, N] fp32, lengths [Bd, N]
 *             int64.  No attentions: none of these decoders exports any.
 * House rules of every entry, those of neuroir_beam.h: enqueued on `stream`; never synchronises, allocates nothing; the same inputs give the
 * same bits; bad arguments return NIR_ERR_BAD_ARG and a short workspace NIR_ERR_WORKSPACE, with nothing enqueued; Bd == 0 (rows == 0) enqueues
 * nothing and returns 0 once the arguments pass, whatever the workspace (it may be NULL).
 * ------------------------------------------------------------------------------------------------ */

/* One sampling step over all of [0, VT) on rows that are ALREADY split, h16 [rows][K/8][2 terms][8] fp16 (the folded LSTM step's output
 * format): token [rows] int32, logp [rows] fp32, lse [rows] fp32 (optional).  No freeze, no feedback.  The counterpart of
 * nir_beam_hredqs_gen_topk: sample_gen_kernel on the split rows (16-byte copies into the LDS planes, no fp32 load, no conversion; one
 * workgroup per CU, the row blocks of a vocabulary range on one XCD) + the finish of nir_sample_gen.  Fast form only: gen_frag
 * (nir_seq2seq_pack_gen_frag of gen_w [VT, K]) is required, K a multiple of 32 in [32, 1024], 0 < VT < 2^31 - 16.  gen_b may be NULL. */
size_t nir_sample_hredqs_gen_workspace_bytes(int64_t rows, int K, int64_t VT);
int nir_sample_hredqs_gen(const void* h16, int64_t rows, int64_t nsrc, int K, const float* gen_b, const void* gen_frag, int64_t VT,
                          float inv_temperature, uint64_t seed, int64_t step, void* workspace, size_t workspace_bytes, int32_t* token, float* logp,
                          float* lse, nir_stream_t stream);

/* HredQS: the arguments of nir_hredqs_decode_greedy plus N, top_k, inv_temperature, seed and the four outputs.  Fast form (all three packs,
 * H % 32 == 0, H <= 1024, tunable exact_f32 off): the folded step, then top_k = 0: the kernel above on the state the step leaves; top_k > 0:
 * nir_beam_hredqs_gen_topk + nir_sample_topk_select's kernel.  Plain form otherwise: the fp32 step, then nir_sample_gen's plain form or
 * nir_beam_gen_topk's plain lists. */
size_t nir_sample_hredqs_decode_workspace_bytes(int64_t B, int64_t S, int N, int top_k, int max_len, const nir_hredqs_decoder_weights* w /*host*/);
int nir_sample_hredqs_decode(const float* h_steps, const float* c_steps, int64_t B, int64_t S, const float* table, int64_t V, int E,
                             const int64_t* tgt2src, int64_t bos, int max_len, const nir_hredqs_decoder_weights* w /*host*/, int N, int top_k,
                             float inv_temperature, uint64_t seed, void* workspace, size_t workspace_bytes, int64_t* predictions,
                             float* token_logprobs, float* scores, int64_t* lengths, nir_stream_t stream);

/* The decoders without attention (M_MATCH_TENSOR, MNSRF): the arguments of nir_beam_plain_decode with N, top_k, inv_temperature, seed in the
 * place of W, and token_logprobs.  The step is that entry's (folded with gate_fold and whh_frag, else fp32); the tail is nir_sample_gen on
 * the fp32 state rows (fused when gen_frag is given), or nir_beam_gen_topk + the selection.  `folded` / `fused` of the size query: whether
 * the packs will be given. */
size_t nir_sample_plain_decode_workspace_bytes(int64_t Bd, int H, int64_t VT, int N, int top_k, int max_len, int folded, int fused);
int nir_sample_plain_decode(const float* dec_h, const float* dec_c, int64_t Bd, int H, const float* table, int64_t V, int E, const float* w_ih,
                            const float* w_hh, const float* b_ih, const float* b_hh, const float* gen_w, const float* gen_b, int64_t VT,
                            const int64_t* tgt2src, int64_t bos, int max_len, const float* gate_fold, const void* whh_frag, const void* gen_frag,
                            int N, int top_k, float inv_temperature, uint64_t seed, void* workspace, size_t workspace_bytes,
                            int64_t* predictions, float* token_logprobs, float* scores, int64_t* lengths, nir_stream_t stream);

/* CARS: the arguments of nir_beam_cars_decode likewise.  Per step that entry's chain -- step, optional query projection, attention,
 * out-projection with tanh, pred1 plus the session term -- and the sampling tail on p1 [R, P] against pred2_w (no bias). */
size_t nir_sample_cars_decode_workspace_bytes(int64_t rows_src, int64_t Bd, int QL, int N, int top_k, int max_len,
                                              const nir_cars_decoder_weights* w /*host*/, int fused);
int nir_sample_cars_decode(const float* dec_h, const float* dec_c, const float* encoded_source, const int64_t* source_len, int64_t rows_src, int QL,
                           const int64_t* rowmap, int64_t Bd, const float* session_cat, const float* table, int64_t V, int E,
                           const int64_t* tgt2src, int64_t bos, int max_len, const nir_cars_decoder_weights* w /*host*/, const void* gen_frag, int N,
                           int top_k, float inv_temperature, uint64_t seed, void* workspace, size_t workspace_bytes, int64_t* predictions,
                           float* token_logprobs, float* scores, int64_t* lengths, nir_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
