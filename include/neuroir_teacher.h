/* libneuroir_hip: the teacher-forced decoder pass of the session models -- Luong attention for many decoder rows that share one memory bank.
 * Included by neuroir_hip.h (which defines the types used here); not meant to be included on its own.  csrc/tf_attend.hip; DESIGN.md section 27. */
#ifndef NEUROIR_TEACHER_H
#define NEUROIR_TEACHER_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * h [ngroups G, H]: the decoder states of ALL teacher-forced steps of all candidates; row r belongs to group g = r / G and reads bank row
 * src = rowmap ? rowmap[g] : g of score_bank / memory_bank [rows_src, QL, H] and source_len[src].  Per row the general / dot forms of
 * nir_seq2seq_attend:
 *   align_j = h . score_bank[src, j, :];  positions j >= clamp(len, 0, QL) masked;  a = softmax(align)
 *   cat[r] = [sum_j a_j memory_bank[src, j, :] ; h[r]]                                                     cat [ngroups G, 2H]
 *   attn (optional, may be NULL): row r at attn + r attn_stride, [QL]; masked positions are exactly 0.0
 * A row of length 0 is NaN throughout (context and attention row), like the reference's softmax over an all -inf row.  score_bank ==
 * memory_bank is the dot form (one bank); the mlp form is not built.
 * A rowmap entry outside [0, rows_src) is CLAMPED into the range: such a group reads a bank row that exists (nothing is read out of bounds)
 * and nothing is flagged -- the callers of this library build the map themselves.
 * Two forms.  Fused (nir_tf_attend_fusable(QL, H, same_bank), G >= 128 and tunable exact_f32 off): one workgroup per (group, block of at most 64
 * rows) splits both banks into two fp16 term planes in LDS once and runs S = h sb^T and ctx = P mem as three v_mfma_f32_16x16x32_f16 per
 * product block, mask and softmax in fp32 registers between them; a bank is staged ceil(G / 64) times instead of being read G times and no
 * [rows, QL, H] intermediate exists.  It needs |h|, |banks| < 2^15 (the split's range).  nir_tf_attend_fusable is the one place that
 * states the shape rule: H a multiple of 32 in [32, 1024], QL <= 64, and both banks next to the workgroup's probability tiles within the
 * CU's 160 KiB of LDS (H 512: QL <= 32; H 1024: QL <= 16).
 * Plain (every other shape with H % 4 == 0 and QL <= 4096, groups of fewer than 128 rows -- measured: below two full row blocks a group
 * the plain form's L2-resident bank reads beat staging the bank --, and everything under exact_f32): one wave per row, fp32 VALU.
 * nir_tf_attend_workspace_bytes is 0 for every shape today (neither form needs scratch); a caller passes what it returns.
 * House rules: enqueued on `stream`, no synchronisation, no allocation, no atomics, the same inputs give the same bits.  Bad arguments (null
 * h / banks / source_len / cat, negative ngroups or G, ngroups G >= 2^31, rows_src <= 0 with rows to do, H outside [4, 8192] or no multiple
 * of 4, QL outside [1, 4096], attn given with attn_stride < QL) return NIR_ERR_BAD_ARG, a workspace shorter than the query's answer
 * NIR_ERR_WORKSPACE, with nothing enqueued; ngroups == 0 or G == 0 enqueues nothing and returns 0.
 * ------------------------------------------------------------------------------------------------ */
int nir_tf_attend_fusable(int QL, int H, int same_bank);
size_t nir_tf_attend_workspace_bytes(int64_t ngroups, int64_t G, int QL, int H);
int nir_tf_attend(const float* h, const float* memory_bank, const float* score_bank, const int64_t* source_len, const int64_t* rowmap,
                  int64_t ngroups, int64_t G, int64_t rows_src, int QL, int H, float* cat, float* attn, int64_t attn_stride, void* workspace,
                  size_t workspace_bytes, nir_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
