/* libneuroir_hip: sampling decode for the Seq2seq recommenders (LSTM and GRU decoders) -- fused generator + Gumbel arg-max.  Included by
 * neuroir_hip.h (which defines the types used here); not meant to be included on its own.  csrc/sample.hip; DESIGN.md section 28. */
#ifndef NEUROIR_SAMPLE_H
#define NEUROIR_SAMPLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * The reference has no sampler; the semantics are this project's, and they mirror include/neuroir_beam.h wherever the two can agree.
 *   rows      N >= 1 samples per source row.  Decode rows R = B N, row r = n B + b (sample n of source row b): the beam's layout
 *             (repeat_beam_size_times).  The memory bank and source_len are NOT repeated (nsrc = B).
 *   noise     counter-based, a pure function of (seed, step t, source row b, sample n, vocabulary id v):
 *               Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (v >> 2, b, t, n); word v & 3 of the output belongs to v;
 *               u = ((word >> 9) + 0.5) 2^-23  (u and 1 - u are exact in fp32);   g = -log(-log u).
 *             Nothing else enters: not the launch geometry, the vocabulary range count, the row tiles of a workgroup, the order of the
 *             partials or the dispatch form.  Keyed by (b, n), not r: a source row's draws do not depend on the batch it sits in.  One Philox
 *             call covers the four logits v0 .. v0 + 3 a lane holds for a row of a tile.  Known answers (the Random123 vectors):
 *               counter 0, key 0                  -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *               counter all-ones, key all-ones    -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *   choice    token = argmax_v fmaf(y[v], 1 / tau, g[v]) in fp32, ties to the smaller v: by the Gumbel-max identity an exact draw from
 *             softmax(y / tau).  y is the biased logit exactly as the greedy kernel forms it.  top_k = 0: over all of [0, VT).  top_k = K in
 *             1 .. NIR_BEAM_MAX_W (K <= VT): over the K largest y (nir_beam_gen_topk's order and tie rule) WITH THE SAME NOISE FUNCTION KEYED
 *             BY v -- the top-k form is the full form restricted to a subset; top_k = 1 is the greedy token for every seed and tau.  tau is
 *             finite and > 0; the entries take inv_temperature = 1 / tau.
 *   logp      y[token] - lse(y): the model's own log-probability at tau = 1 over the full vocabulary, whatever tau and top_k are, so that
 *             scores compare across settings and score_candidates([BOS] + sample) reproduces them.
 *             (A whole-vocabulary draw can emit PAD (0) like any id; nir_score_sequences does not count a PAD position, so the round trip
 *             holds for samples without PAD in front of their first EOS -- otherwise it returns the score less those positions.)
 *   freeze    a row whose last token was EOS (NIR_BEAM_EOS = 3) emits EOS at log-probability 0 from then on; scores is the fp32 sum in step
 *             order; lengths is the index of the first EOS + 1, else max_len.
 *   feedback  the next input id is tgt2src[token] (the token itself without a table), <unk> (1) outside [0, V), like the greedy decode.
 *   horizon   max_len steps, no early stop, no host synchronisation.
 *   outputs   in sample order (i.i.d., not sorted, duplicates possible): predictions [B, N, max_len] int64, token_logprobs [B, N, max_len]
 *             fp32 (0 behind EOS), scores [B, N] fp32, lengths [B, N] int64, attentions [B, N, max_len, QL] fp32.
 * House rules of every entry, those of neuroir_beam.h: enqueued on `stream`; never synchronises, allocates nothing; the same inputs give the
 * same bits; bad arguments return NIR_ERR_BAD_ARG and a short workspace NIR_ERR_WORKSPACE, with nothing enqueued; no rows: nothing enqueued.
 * ------------------------------------------------------------------------------------------------ */

/* The noise the kernels add, from the same device function: g [rows, VT] fp32, row r = n nsrc + b reads (b, n) = (r % nsrc, r / nsrc);
 * words (optional) [rows, VT] uint32: the Philox word of every (row, v).  step in [0, 2^32), nsrc >= 1, rows in [0, 2^31), VT in [1, 2^31 - 16). */
int nir_sample_noise(uint64_t seed, int64_t step, int64_t nsrc, int64_t rows, int64_t VT, float* g, uint32_t* words, nir_stream_t stream);

/* One sampling step over all of [0, VT) on given rows x [rows, K]: token [rows] int32, logp [rows] fp32, lse [rows] fp32 (optional).  No
 * freeze, no feedback.  Fused form -- gen_frag given (nir_seq2seq_pack_gen_frag), K a multiple of 32 in [32, 1024], tunable exact_f32 off:
 * sample_gen_kernel keeps (perturbed best, its index, its logit, max, sum) of every row on chip, the logits never leave it.  Plain form
 * otherwise (K % 4 == 0): the fp32 GEMM into [rows, VT] logits in the workspace and one workgroup per row.  `fused` of the workspace query:
 * nonzero when a fragment will be given -- the size is that of the form the entry then runs.  gen_b may be NULL. */
size_t nir_sample_gen_workspace_bytes(int64_t rows, int K, int64_t VT, int fused);
int nir_sample_gen(const float* x, int64_t rows, int64_t nsrc, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                   float inv_temperature, uint64_t seed, int64_t step, void* workspace, size_t workspace_bytes, int32_t* token, float* logp,
                   float* lse, nir_stream_t stream);

/* The top-k form's choice behind nir_beam_gen_topk: per row the W entries (top_val, top_idx) [rows, W] are perturbed with the noise of
 * their vocabulary ids and the best is picked (ties to the smaller id); logp = top_val[pick] - lse[row].  W in 1 .. NIR_BEAM_MAX_W. */
int nir_sample_topk_select(const float* top_val, const int32_t* top_idx, const float* lse, int64_t rows, int64_t nsrc, int W,
                           float inv_temperature, uint64_t seed, int64_t step, int32_t* token, float* logp, nir_stream_t stream);

/* The whole decode: the attention-decoder step of the greedy and beam decodes with the sampling tail behind it.  dec_h, dec_c [B N, H]: the
 * initial state repeated in the layout above; memory_bank [B, QL, H] and source_len [B] are NOT repeated.  The other arguments are those of
 * nir_seq2seq_decode_greedy.  top_k = 0 or 1 .. min(NIR_BEAM_MAX_W, VT); inv_temperature finite and > 0.  B == 0: nothing enqueued and 0
 * returned once the arguments pass, whatever the workspace (it may be NULL). */
size_t nir_sample_seq2seq_decode_workspace_bytes(int64_t B, int QL, int N, int top_k, int max_len, const nir_seq2seq_decoder_weights* w /*host*/);
int nir_sample_seq2seq_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, int N,
                              int top_k, float inv_temperature, uint64_t seed, const float* table, int64_t V, int E, const int64_t* tgt2src,
                              int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w /*host*/, void* workspace, size_t workspace_bytes,
                              int64_t* predictions, float* token_logprobs, float* scores, int64_t* lengths, float* attentions,
                              nir_stream_t stream);
/* The same with the GRU decoder (no cell state; the struct as nir_seq2seq_gru_decode_greedy reads it). */
size_t nir_sample_seq2seq_gru_decode_workspace_bytes(int64_t B, int QL, int N, int top_k, int max_len,
                                                     const nir_seq2seq_decoder_weights* w /*host*/);
int nir_sample_seq2seq_gru_decode(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, int N, int top_k,
                                  float inv_temperature, uint64_t seed, const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos,
                                  int max_len, const nir_seq2seq_decoder_weights* w /*host*/, void* workspace, size_t workspace_bytes,
                                  int64_t* predictions, float* token_logprobs, float* scores, int64_t* lengths, float* attentions,
                                  nir_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
