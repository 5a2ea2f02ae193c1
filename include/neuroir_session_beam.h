/* libneuroir_hip: beam search for the session models (CARS, M_MATCH_TENSOR, MNSRF).  Included by neuroir_hip.h (which defines the types used
 * here); not meant to be included on its own.  csrc/beam.hip. */
#ifndef NEUROIR_SESSION_BEAM_H
#define NEUROIR_SESSION_BEAM_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * The search is the one of neuroir_beam.h (DESIGN.md sections 21 and 23) with "source row" read as "decode row of the greedy decode":
 * Bd = B (S-1) source rows, R = Bd W beam rows, row = k Bd + i (beam k of decode row i).  Step 0 has only beam 0 live; a live beam offers
 * cum + (logit - lse), a finished beam (k, EOS) alone at its frozen score; the W best by (score descending, flat index k VT + v ascending);
 * feedback tgt2src[v], <unk> (1) outside [0, V); max_len steps, no early stop, no length normalisation, no coverage.  W = 1 is the greedy decode
 * token for token until a row emits EOS.
 * The caller does NOT repeat anything: dec_h / dec_c [Bd, H], and for CARS rowmap [Bd], encoded_source, source_len and session_cat, are the greedy
 * entry's arguments; beam row r reads what decode row r % Bd reads.
 * Outputs, backtracked through the stored back-pointers, best beam first: predictions [Bd, W, max_len] int64 (EOS repeated after the first EOS),
 * scores [Bd, W] fp32, lengths [Bd, W] int64 (index of the first EOS + 1, else max_len), backptr (optional) [max_len, Bd, W] int32 (the
 * workspace size covers a call without it).  No attention output: the CARS greedy decode exports none either.
 * gen_frag (optional): nir_seq2seq_pack_gen_frag of the generator weight -- token_prob_predictor2.weight [VT, P] (K = P, no bias) for CARS,
 * generator.weight [VT, H] (K = H) for the plain decoders.  With it, K a multiple of 32 in [32, 1024] and tunable exact_f32 off the generator,
 * the log-sum-exp and the top-W run as ONE kernel per step (beam_gen_topk_kernel) and no [R, VT] logits are written; otherwise the fp32 GEMM
 * into workspace logits + beam_row_topk_kernel.  (CARS' pred2_frag of the greedy arg-max is not read here.)
 * House rules as in neuroir_beam.h: enqueued on `stream`, no synchronisation, no allocation, the same inputs give the same bits; bad arguments
 * (W outside 1..NIR_BEAM_MAX_W, VT < W, null pointers, bad dims) return NIR_ERR_BAD_ARG and a short workspace NIR_ERR_WORKSPACE, with nothing
 * enqueued; Bd == 0 enqueues nothing, in every form.  `fused` of the size queries: whether gen_frag will be given.
 * ------------------------------------------------------------------------------------------------ */

/* CARS: the arguments of nir_cars_decode_greedy plus W and gen_frag. */
size_t nir_beam_cars_decode_workspace_bytes(int64_t rows_src, int64_t Bd, int QL, int W, int max_len, const nir_cars_decoder_weights* w /*host*/,
                                            int fused);
int nir_beam_cars_decode(const float* dec_h, const float* dec_c, const float* encoded_source, const int64_t* source_len, int64_t rows_src, int QL,
                         const int64_t* rowmap, int64_t Bd, const float* session_cat, const float* table, int64_t V, int E, const int64_t* tgt2src,
                         int64_t bos, int max_len, const nir_cars_decoder_weights* w /*host*/, const void* gen_frag, int W, void* workspace,
                         size_t workspace_bytes, int64_t* predictions, float* scores, int64_t* lengths, int32_t* backptr, nir_stream_t stream);

/* The decoders without attention (M_MATCH_TENSOR, MNSRF): the arguments of nir_decode_greedy_plain_folded plus W and gen_frag. */
size_t nir_beam_plain_decode_workspace_bytes(int64_t Bd, int H, int64_t VT, int W, int max_len, int folded, int fused);
int nir_beam_plain_decode(const float* dec_h, const float* dec_c, int64_t Bd, int H, const float* table, int64_t V, int E, const float* w_ih,
                          const float* w_hh, const float* b_ih, const float* b_hh, const float* gen_w, const float* gen_b, int64_t VT,
                          const int64_t* tgt2src, int64_t bos, int max_len, const float* gate_fold, const void* whh_frag, const void* gen_frag, int W,
                          void* workspace, size_t workspace_bytes, int64_t* predictions, float* scores, int64_t* lengths, int32_t* backptr,
                          nir_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
