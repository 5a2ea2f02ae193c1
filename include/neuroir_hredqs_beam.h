/* libneuroir_hip: beam search for HredQS (the hierarchical recurrent encoder-decoder for query suggestion).  Included by neuroir_hip.h (which
 * defines the types used here); not meant to be included on its own.  csrc/beam.hip. */
#ifndef NEUROIR_HREDQS_BEAM_H
#define NEUROIR_HREDQS_BEAM_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * The search is the one of neuroir_beam.h and neuroir_session_beam.h (DESIGN.md sections 21, 23 and 25) with "source row" read as "decode row of
 * nir_hredqs_decode_greedy": Bd = B S source rows, one per session prefix, in (b, s) order; R = Bd W beam rows, row = k Bd + i (beam k of source
 * row i).  The initial state of source row i is the state of session step i / B of session i % B -- the reference's pairing, applied by the
 * entry itself to SOURCE rows (h_steps / c_steps [B, S, H] are the greedy entry's arguments; nothing is paired or repeated by the caller).
 * Step 0 has only beam 0 live; a live beam offers cum + (logit - lse), a finished beam (k, EOS) alone at its frozen score; the W best by (score
 * descending, flat index k VT + v ascending); feedback tgt2src[v], <unk> (1) outside [0, V); max_len steps, no early stop, no length
 * normalisation, no coverage.  W = 1 is the greedy decode token for token until a row emits EOS.
 * Outputs, backtracked through the stored back-pointers, best beam first: predictions [B, S, W, max_len] int64 (EOS repeated after the first EOS),
 * scores [B, S, W] fp32, lengths [B, S, W] int64 (index of the first EOS + 1, else max_len), backptr (optional) [max_len, Bd, W] int32 (the
 * workspace size covers a call without it).  There are no attentions.
 * Two forms, as the greedy entry has.  Fast: all three packs of nir_hredqs_decoder_weights given, H a multiple of 32 up to 1024, tunable
 * exact_f32 off -- per step the folded LSTM step, the generator + bias + log-sum-exp + top-W on the split state the step leaves
 * (beam_gen_topk_kernel on BeamRowsSplit: no fp32 row is read and no [R, VT] logits are written), select, reorder.  Plain otherwise: the fp32 step, the fp32
 * GEMM into workspace logits, beam_row_topk_kernel, select, reorder.
 * House rules as in neuroir_beam.h: enqueued on `stream`, no synchronisation, no allocation, the same inputs give the same bits; bad arguments
 * (W outside 1..NIR_BEAM_MAX_W, VT < W, null pointers, bad dims) return NIR_ERR_BAD_ARG and a short workspace NIR_ERR_WORKSPACE, with nothing
 * enqueued; B S == 0 (rows == 0) enqueues nothing, in every form.
 * ------------------------------------------------------------------------------------------------ */

/* Per row of the split state h16 [rows][K/8][2 terms][8] (fp16 term pairs, the folded LSTM step's output format): lse and the W largest of
 * gen_w h + gen_b with their indices (value descending, index ascending among equals) -- top_val / top_idx [rows, W], lse [rows].  gen_frag:
 * nir_seq2seq_pack_gen_frag of gen_w [VT, K]; gen_b [VT] or NULL.  K a multiple of 32 in [32, 1024], 0 < VT < 2^31 - 16. */
size_t nir_beam_hredqs_gen_topk_workspace_bytes(int64_t rows, int K, int64_t VT, int W);
int nir_beam_hredqs_gen_topk(const void* h16, int64_t rows, int K, const float* gen_b, const void* gen_frag, int64_t VT, int W, void* workspace,
                             size_t workspace_bytes, float* top_val, int32_t* top_idx, float* lse, nir_stream_t stream);

/* The arguments of nir_hredqs_decode_greedy plus W, the scores, the lengths and the optional back-pointers. */
size_t nir_beam_hredqs_decode_workspace_bytes(int64_t B, int64_t S, int W, int max_len, const nir_hredqs_decoder_weights* w /*host*/);
int nir_beam_hredqs_decode(const float* h_steps, const float* c_steps, int64_t B, int64_t S, const float* table, int64_t V, int E,
                           const int64_t* tgt2src, int64_t bos, int max_len, const nir_hredqs_decoder_weights* w /*host*/, int W, void* workspace,
                           size_t workspace_bytes, int64_t* predictions, float* scores, int64_t* lengths, int32_t* backptr, nir_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
