/* libneuroir_hip: beam search for the Seq2seq recommenders (LSTM and GRU decoders).  Included by neuroir_hip.h (which defines the types used
 * here); not meant to be included on its own.  csrc/beam.hip. */
#ifndef NEUROIR_BEAM_H
#define NEUROIR_BEAM_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * The reference ships the state helpers of a beam and no search: neuroir/decoders/state.py:16-31 (beam_update) and :65-69
 * (repeat_beam_size_times).  They fix the row layout and the state shuffle; the search itself is this project's:
 *   width    1 <= W <= NIR_BEAM_MAX_W, VT >= W.  Decode rows R = B W, row = k B + b (beam k of source row b), as repeat_beam_size_times lays
 *            them out.  A reorder of source row b is new[k] = old[backptr[b, k]], which is beam_update(b, positions, W).
 *   step 0   only beam 0 is live: cum[b] = (0, -inf, ..., -inf).
 *   offers   live beam k offers cum[b, k] + (logit[v] - lse(row)) for every v (fp32, in this order); a finished beam (its last token was EOS,
 *            NIR_BEAM_EOS = 3) offers exactly one candidate, (k, EOS), at cum[b, k] unchanged.
 *   select   the W best of the W VT candidates of a source row, in descending score order; ties go to the smaller flat index k VT + v.
 *   feedback the next input id is tgt2src[v] (v itself without a table), <unk> (1) outside [0, V), like the greedy decode.
 *   horizon  max_len steps, no early stop, fixed shapes, no host synchronisation; a score stays frozen after EOS.
 * No length normalisation, no coverage penalty.
 * House rules of every entry: enqueued on `stream`; never synchronises, allocates nothing; the same inputs give the same bits; bad arguments
 * (W outside 1..8, VT < W, null pointers) return NIR_ERR_BAD_ARG and a short workspace NIR_ERR_WORKSPACE, with nothing enqueued.
 * ------------------------------------------------------------------------------------------------ */
#define NIR_BEAM_MAX_W 8
#define NIR_BEAM_EOS 3

/* Per decode row: the W largest logits y[v] = x[row, :] . gen_w[v, :] + gen_b[v] (descending, the smaller index first among equals) and
 * lse = log sum_v exp(y[v]).  x [rows, K]; top_val [rows, W] fp32, top_idx [rows, W] int32, lse [rows] fp32.
 * Fused form -- gen_frag given (nir_seq2seq_pack_gen_frag), K a multiple of 32 in [32, 1024], tunable exact_f32 off: the logits never leave
 * the chip (split-fp16 MFMA as in the greedy generator; every lane keeps an online-softmax pair and a sorted top-W list).  Plain form
 * otherwise (K % 4 == 0): the fp32 GEMM into [rows, VT] logits in the workspace and one workgroup per row.  gen_b may be NULL.  rows == 0:
 * nothing enqueued. */
size_t nir_beam_gen_topk_workspace_bytes(int64_t rows, int K, int64_t VT, int W, int fused);
int nir_beam_gen_topk(const float* x, int64_t rows, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT, int W,
                      void* workspace, size_t workspace_bytes, float* top_val, int32_t* top_idx, float* lse, nir_stream_t stream);

/* One selection step for B source rows from the per-row results above (rows = B W in the layout k B + b).  cum [B, W] fp32 and finished
 * [B, W] int32 are read and updated in place; backptr [B, W] int32, token [B, W] int32 (target-vocabulary ids) and next_ids [B W] int64 (row
 * order k B + b, mapped through tgt2src, which may be NULL) are written. */
int nir_beam_select(const float* top_val, const int32_t* top_idx, const float* lse, int64_t B, int W, int64_t VT, const int64_t* tgt2src, int64_t V,
                    float* cum, int32_t* finished, int32_t* backptr, int32_t* token, int64_t* next_ids, nir_stream_t stream);

/* The state shuffle in one launch: row k B + b of every output is row backptr[b, k] B + b of its input, for h [B W, H], c (both NULL for a
 * GRU) and the fp16 term-pair state h16 [B W][H/8][2][8] (both NULL without the fp16-term step; H % 8 == 0 with it) -- bit for bit a gather of
 * the fp32 state followed by the pack.  H % 4 == 0; no output may alias an input. */
int nir_beam_reorder(const int32_t* backptr, int64_t B, int W, int H, const float* h_in, float* h_out, const float* c_in, float* c_out,
                     const void* h16_in, void* h16_out, nir_stream_t stream);

/* The whole search.  dec_h, dec_c [B W, H]: the initial state repeated in the layout above; memory_bank [B, QL, H] and source_len [B] are NOT
 * repeated.  The other arguments are those of nir_seq2seq_decode_greedy.  Outputs, all backtracked through the stored back-pointers, best
 * beam first: predictions [B, W, max_len] int64 (EOS repeated after the first EOS), scores [B, W] fp32, lengths [B, W] int64 (index of the
 * first EOS + 1, else max_len), attentions [B, W, max_len, QL] fp32.  backptr (optional) [max_len, B, W] int32: every step's back-pointers
 * (the workspace size covers a call without it).  B == 0: nothing enqueued, in every form. */
size_t nir_beam_seq2seq_decode_workspace_bytes(int64_t B, int QL, int W, int max_len, const nir_seq2seq_decoder_weights* w /*host*/);
int nir_beam_seq2seq_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, int W,
                            const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                            const nir_seq2seq_decoder_weights* w /*host*/, void* workspace, size_t workspace_bytes, int64_t* predictions,
                            float* scores, int64_t* lengths, float* attentions, int32_t* backptr, nir_stream_t stream);
/* The same with the GRU decoder (no cell state; the struct as nir_seq2seq_gru_decode_greedy reads it). */
size_t nir_beam_seq2seq_gru_decode_workspace_bytes(int64_t B, int QL, int W, int max_len, const nir_seq2seq_decoder_weights* w /*host*/);
int nir_beam_seq2seq_gru_decode(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, int W,
                                const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                                const nir_seq2seq_decoder_weights* w /*host*/, void* workspace, size_t workspace_bytes, int64_t* predictions,
                                float* scores, int64_t* lengths, float* attentions, int32_t* backptr, nir_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
