/* libneuroir_hip: teacher-forced scoring of candidate queries -- the generator's log-likelihood of given target tokens, without the logits.
 * Included by neuroir_hip.h (which defines the types used here); not meant to be included on its own.  csrc/score.hip; DESIGN.md section 26. */
#ifndef NEUROIR_SCORE_H
#define NEUROIR_SCORE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * Per row r of x [rows, K] (the decoder outputs of ALL time steps of all candidates at once) with logits y = gen_w x[r] + gen_b:
 *   lse[r] = log sum_v exp(y[v]),   token_logp[r] = y[target[r]] - lse[r]
 * token_logp [rows] is written for every row: 0 where target[r] == pad, and 0 where target[r] lies outside [0, VT) -- that case also ORs bit 0
 * into *id_flag when one is given (the word nir_softmax_nll_ent_fwd sets).  lse [rows] may be NULL.
 * Two forms.  Fused: gen_frag (nir_seq2seq_pack_gen_frag of gen_w [VT, K]) given, K a multiple of 32 in [32, 1024], tunable exact_f32 off --
 * score_gen_target_kernel keeps (max, sum, the target's logit) of every row on chip and a finish kernel merges the partials; no [rows, VT]
 * tensor exists.  Plain otherwise: the fp32 GEMM into workspace logits in row chunks of at most 256 MiB of logits (a single row where a row is
 * larger), one workgroup per row behind it.  `fused` of the workspace query: nonzero when a fragment will be given -- the size is that of the
 * form the entry then runs (the plain one where K, VT or the tunable rule the fused one out).  Rows beyond 2^18 run in chunks of 2^18 rows on
 * the host, so no launch exceeds the grid limits and the workspace is bounded by one chunk's.
 * House rules: enqueued on `stream`, no synchronisation, no allocation, no float atomics, the same inputs give the same bits.  Bad arguments
 * (null x / gen_w / target / token_logp, rows outside [0, 2^31), K outside [4, 8192] or no multiple of 4, VT outside [1, 2^31 - 16)) return
 * NIR_ERR_BAD_ARG and a null or short workspace NIR_ERR_WORKSPACE, with nothing enqueued; rows == 0 enqueues nothing and returns 0.
 * ------------------------------------------------------------------------------------------------ */
size_t nir_score_gen_target_workspace_bytes(int64_t rows, int K, int64_t VT, int fused);
int nir_score_gen_target(const float* x, int64_t rows, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                         const int64_t* target, int64_t pad, void* workspace, size_t workspace_bytes, float* token_logp, float* lse, int32_t* id_flag,
                         nir_stream_t stream);

/* Rows [nseq][T] of token log-probabilities and their targets -> per sequence the sum and the number of the positions that count.  Position j
 * counts iff target[j] != pad, target[j] >= 0 (an id past the vocabulary is nir_score_gen_target's to flag; its log-probability is 0) and no
 * EARLIER position of the sequence held eos: the beam's "frozen at EOS" rule, so a beam's predictions row -- EOS repeated behind the first EOS --
 * is scored as it is.  scores [nseq] fp32: the sum in position order; lengths [nseq] int64; the positions of token_logp that do not count are
 * set to 0 in place.  eos < 0: no token ends a sequence.  Bad arguments (null pointers, nseq < 0, T <= 0 or > 2^20) return NIR_ERR_BAD_ARG;
 * nseq == 0 enqueues nothing. */
int nir_score_sequences(float* token_logp, const int64_t* target, int64_t nseq, int T, int64_t pad, int64_t eos, float* scores, int64_t* lengths,
                        nir_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
