/* libneuroir_hip: sampling decode for ACG, the Seq2seq recommender with a copy generator (LSTM and GRU decoders) -- draws from the collapsed
 * extended distribution, without the logits and without a dense copy distribution.  Included by neuroir_hip.h (which defines the types used
 * here); not meant to be included on its own.  csrc/sample.hip; DESIGN.md section 33. */
#ifndef NEUROIR_ACG_SAMPLE_H
#define NEUROIR_ACG_SAMPLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * The reference has no sampler; the semantics are this project's.  The noise function, the row layout, the freeze rule, the horizon and the
 * outputs are those of neuroir_sample.h; the candidate set and P are those of neuroir_acg_beam.h.  Restated here is only what is new.
 *   rows      R = B N decode rows, row r = n B + b.  The memory bank, source_len, src_map_idx [B, QL], ext2tgt [B, CV] and ext2src [B, CV] are
 *             NOT repeated: row r reads source row r % B.
 *   P(e)      exactly neuroir_acg_beam.h's, by EXTENDED id e in [0, VT + CV), in the fp32 expressions of nir_acg_gen_select (l[PAD] := -1e-20
 *             behind the linear, m = max l, Z = sum exp(l - m), z = sigmoid(x), 1 - z = sigmoid(-x), mass[c] = z sum_{j < len[b], map[b, j] = c}
 *             a[r, j], j ascending): a word no slot collapses onto has (1 - z) exp(l[v] - m) / Z; a collapse target is offered ONCE, with its
 *             slots' mass added; a slot that is not collapsed has mass[c]; a collapsed slot is no candidate and is never drawn.
 *   noise     neuroir_sample.h's function keyed by the EXTENDED id: counter (e >> 2, b, t, n), word e & 3.  nir_sample_noise with VT := VT + CV
 *             therefore returns exactly what the kernels add.
 *   choice    token = argmax_e (log P(e) / tau + g[e]), ties to the smaller e: by the Gumbel-max identity an exact draw from P^(1/tau)
 *             normalised over the candidates.  P = 0 gives -inf and is never chosen (a row none of whose candidates has positive probability
 *             emits id 0).  In fp32 the kernels evaluate
 *               a word no slot collapses onto     fmaf(l[v], 1/tau, g[v]) + c_row,   c_row = (logf(1 - z) - m - logf(Z)) / tau
 *               a target, a slot                  fmaf(logf(P), 1/tau, g[e])
 *             A target's l[t] is the fp32 row dot behind the fused walk and the GEMM's own logit in the plain forms.
 *   top_k     K in 1 .. min(NIR_BEAM_MAX_W, VT): the same choice over the K largest P of the row (nir_acg_beam_gen_select's list and tie rule),
 *             every entry as fmaf(logf(P), 1/tau, g[e]) with the same noise keyed by e.  top_k = 1 is nir_acg_decode_greedy's token for every
 *             seed and tau.
 *   logp      logf(P(token)): the model's own log-probability at tau = 1 over the full collapsed distribution, whatever tau and top_k are, so
 *             nir_acg_score_gen_target on [BOS] + sample reproduces scores and lengths.  neuroir_sample.h's PAD caveat carries over, and PAD
 *             has real mass under ACG (its logit is about zero): nir_score_sequences does not count a PAD position.
 *   feedback  tgt2src[e] (e itself without a table) below VT, ext2src[b, e - VT] from VT on; <unk> (1) outside [0, V).
 *   outputs   as neuroir_sample.h, with EXTENDED ids in predictions; attentions is the decoder's own attention, as in the greedy decode.
 * Why 1 + CV candidates per row suffice (neuroir_acg_beam.h's argument for W = 1, under noise).  Every collapse target and every slot is
 * evaluated exactly.  Among the words no slot collapses onto the perturbed value is fmaf(l, 1/tau, g) plus the row constant c_row, so their
 * best is the generator walk's perturbed winner over ALL of [0, VT) -- unless that winner is a target.  If it is, its exact value (mass
 * added) is at least its raw value and still dominates every such word.  So the draw is the maximum over the raw perturbed winner (dropped
 * when it is a target), every target and every slot that is not collapsed; neither [rows, VT] logits nor a [rows, VT + CV] distribution is
 * written.
 * Limits: QL in [1, 4096], CV in [2, 1024], VT + CV < 2^31 - 16.
 * House rules of every entry, those of neuroir_beam.h: enqueued on `stream`; never synchronises, allocates nothing; no atomics, every
 * reduction in a fixed order: the same inputs give the same bits; bad arguments return NIR_ERR_BAD_ARG and a null or short workspace
 * NIR_ERR_WORKSPACE, with nothing enqueued and no output touched; no rows: nothing enqueued.
 * ------------------------------------------------------------------------------------------------ */

/* One draw per row on given rows: o [rows, K] attentional outputs, copy_attn row r at copy_attn + r * attn_stride, [QL]; row r = n nsrc + b
 * reads source_len [nsrc], src_map_idx [nsrc, QL], ext2tgt [nsrc, CV] of source row b (ext2src [nsrc, CV] is not read: there is no feedback
 * here).  token [rows] int32 (extended ids), logp [rows] fp32.  No freeze, no feedback.  top_k = 0: over the whole collapsed distribution --
 * fused form (gen_frag given, K a multiple of 32 in [32, 1024], tunable exact_f32 off): the PAD-substituting sample_gen_kernel keeps (perturbed
 * best, its id, its logit, max, sum) on chip; plain form otherwise (K % 4 == 0): the fp32 GEMM into workspace logits and one workgroup per
 * row; acg_sample_row_kernel (one wave per row) behind either.  gen_max / gen_lse [rows] fp32 (optional): m and m + log Z of the PAD-substituted
 * logits, written by this form.  top_k = K: nir_acg_beam_gen_select's lists (either of its forms) and the top-k select on (log P, e); gen_max
 * and gen_lse must be NULL.  `fused` of the workspace query: nonzero when a fragment will be given.  step in [0, 2^32), 1 <= nsrc <= rows. */
size_t nir_acg_sample_gen_select_workspace_bytes(int64_t rows, int K, int64_t VT, int top_k, int fused);
int nir_acg_sample_gen_select(const float* o, int64_t rows, int64_t nsrc, int K, const float* gen_w, const float* gen_b, const void* gen_frag,
                              int64_t VT, int top_k, float inv_temperature, uint64_t seed, int64_t step, const float* copy_w, const float* copy_b,
                              const float* copy_attn, int64_t attn_stride, const int64_t* source_len, int QL, const int64_t* src_map_idx,
                              const int64_t* ext2tgt, const int64_t* ext2src, int CV, void* workspace, size_t workspace_bytes, int32_t* token,
                              float* logp, float* gen_max, float* gen_lse, nir_stream_t stream);

/* The whole decode: the arguments of nir_acg_beam_decode with N, top_k, inv_temperature, seed in the place of W, token_logprobs among the
 * outputs and no back-pointers.  dec_h, dec_c [B N, H]: the initial state repeated in the layout above.  The step is the attention decoder's
 * over R rows; with reuse_copy_attn off the copy attention runs over the R rows against the B source rows.  B == 0: nothing enqueued and 0
 * returned once the arguments pass, whatever the workspace (it may be NULL). */
size_t nir_acg_sample_decode_workspace_bytes(int64_t B, int QL, int CV, int N, int top_k, int max_len, const nir_seq2seq_decoder_weights* w /*host*/,
                                             const nir_acg_copy_weights* cw /*host*/);
int nir_acg_sample_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL,
                          const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                          const nir_seq2seq_decoder_weights* w /*host*/, const nir_acg_copy_weights* cw /*host*/, const int64_t* src_map_idx,
                          const int64_t* ext2tgt, const int64_t* ext2src, int CV, int N, int top_k, float inv_temperature, uint64_t seed,
                          void* workspace, size_t workspace_bytes, int64_t* predictions, float* token_logprobs, float* scores, int64_t* lengths,
                          float* attentions, nir_stream_t stream);
/* The same with the GRU decoder (no cell state). */
size_t nir_acg_sample_gru_decode_workspace_bytes(int64_t B, int QL, int CV, int N, int top_k, int max_len,
                                                 const nir_seq2seq_decoder_weights* w /*host*/, const nir_acg_copy_weights* cw /*host*/);
int nir_acg_sample_gru_decode(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, const float* table,
                              int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w /*host*/,
                              const nir_acg_copy_weights* cw /*host*/, const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src,
                              int CV, int N, int top_k, float inv_temperature, uint64_t seed, void* workspace, size_t workspace_bytes,
                              int64_t* predictions, float* token_logprobs, float* scores, int64_t* lengths, float* attentions,
                              nir_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
