/* libneuroir_hip: teacher-forced scoring of candidate queries under ACG, the Seq2seq recommender with a copy generator -- the log-probability of
 * given EXTENDED ids under the collapsed extended distribution, without the logits and without a dense copy distribution.  Included by
 * neuroir_hip.h (which defines the types used here); not meant to be included on its own.  csrc/score.hip; DESIGN.md section 31. */
#ifndef NEUROIR_ACG_SCORE_H
#define NEUROIR_ACG_SCORE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * The reference ships no scorer; the semantics are this project's and mirror neuroir_acg_beam.h.  o [rows, K]: the attentional outputs of ALL
 * teacher-forced steps of all candidates, rows in (b, n, t) order; row r reads source row r / rows_per_src of source_len [nsrc], src_map_idx
 * [nsrc, QL] and ext2tgt [nsrc, CV] (nsrc = rows / rows_per_src; the maps are never repeated) and its own copy attention at copy_attn +
 * r * attn_stride, [QL].  target [rows]: EXTENDED ids e in [0, VT + CV) -- what nir_acg_decode_greedy and nir_acg_beam_decode emit.
 * With the quantities of nir_acg_beam_gen_select in its fp32 expressions -- l = W_g o + b_g (l[PAD] := -1e-20 behind the linear), m = max l,
 * Z = sum exp(l - m), z = sigmoid(x), 1 - z = sigmoid(-x), x = w_c . o + b_c, a the row's copy attention read at j < len only, j ascending:
 *   a target word w < VT             P = (1 - z) exp(l[w] - m) / Z + sum{ z a[j] : c = map[j] >= 2, ext2tgt[c] == w }
 *                                    -- the word's generator mass plus the mass of ALL slots that collapse onto it
 *   a slot VT + c, not collapsed     P = sum{ z a[j] : map[j] == c }                    (c < 2, or ext2tgt[c] outside [0, VT))
 *   a collapsed slot VT + c          scored as its word w = ext2tgt[c], to the bit: one word has one probability, however it is spelled.
 *                                    (The reference leaves 1e-10 at the slot and the beam never offers it: the one deliberate difference
 *                                    from the reference's matrix.)
 * token_logp[r] = logf(P); P == 0 gives -inf, as in the beam.  token_logp [rows] is written for every row: 0 where e == pad, 0 where e is
 * negative, and 0 where e >= VT + CV -- that last case also ORs bit 0 into *id_flag when one is given.  map[j] at j >= len is never read; a
 * map entry outside [0, CV) contributes nothing.  nir_score_sequences (neuroir_score.h) runs unchanged behind this entry.
 * Two forms, as in nir_score_gen_target.  Fused: gen_frag (nir_seq2seq_pack_gen_frag) given, K a multiple of 32 in [32, 1024], tunable
 * exact_f32 off -- the PAD-substituting form of score_gen_target_kernel keeps (max, sum, the word's logit) on chip.  Plain otherwise
 * (K % 4 == 0): the fp32 GEMM into workspace logits in row chunks and one workgroup per row.  One finish kernel (a wave per row) behind either:
 * merge, switch, the copy mass as a gather, log P.  No [rows, VT] and no [rows, CV] tensor exists in the fused form.
 * House rules: enqueued on `stream`, no synchronisation, no allocation, no float atomics, the same inputs give the same bits; rows beyond 2^18
 * run in host chunks of 2^18 rows.  Bad arguments (null pointers other than gen_b / gen_frag / id_flag, rows outside [0, 2^31), rows_per_src
 * < 1 or no divisor of rows, K outside [4, 8192] or no multiple of 4, VT outside [1, 2^31 - 16 - 1024), QL outside [1, 4096], CV outside
 * [2, 1024], attn_stride < QL) return NIR_ERR_BAD_ARG and a null or short workspace NIR_ERR_WORKSPACE, with nothing enqueued; rows == 0
 * enqueues nothing and returns 0.
 * ------------------------------------------------------------------------------------------------ */
size_t nir_acg_score_gen_target_workspace_bytes(int64_t rows, int K, int64_t VT, int fused);
int nir_acg_score_gen_target(const float* o, int64_t rows, int64_t rows_per_src, int K, const float* gen_w, const float* gen_b, const void* gen_frag,
                             int64_t VT, const float* copy_w, const float* copy_b, const float* copy_attn, int64_t attn_stride,
                             const int64_t* source_len, int QL, const int64_t* src_map_idx, const int64_t* ext2tgt, int CV,
                             const int64_t* target /*extended ids*/, int64_t pad, void* workspace, size_t workspace_bytes, float* token_logp,
                             int32_t* id_flag, nir_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
