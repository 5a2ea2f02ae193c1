/* libneuroir_hip: corpus retrieval for the two-tower rankers (DSSM, CDSSM) -- a document index of unit rows and a fused cosine top-k over it.
 * A header of its own: NOT included by neuroir_hip.h.  Include neuroir_hip.h first (it defines nir_stream_t and the error codes).
 * csrc/retrieve.hip; DESIGN.md section 34.
 *
 * House rules of every entry: enqueued on `stream`, no synchronisation, no allocation, no float atomics, the same inputs give the same bits.  Bad
 * arguments return NIR_ERR_BAD_ARG and a null or short workspace NIR_ERR_WORKSPACE, with nothing enqueued; a call with no rows (B == 0, m == 0)
 * enqueues nothing and returns 0. */
#ifndef NEUROIR_RETRIEVE_H
#define NEUROIR_RETRIEVE_H

#ifdef __cplusplus
extern "C" {
#endif

#define NIR_RETRIEVE_MAX_K 128
#define NIR_RETRIEVE_MAX_D 256
/* `form` of nir_retrieve_topk and nir_retrieve_topk_workspace_bytes */
#define NIR_RETRIEVE_AUTO 0
#define NIR_RETRIEVE_FUSED 1
#define NIR_RETRIEVE_PLAIN 2

/* ---------------------------------------------------------------------------------------------------
 * The index: `capacity` documents of D components, 1 <= D <= NIR_RETRIEVE_MAX_D, stored as unit rows y / max(|y|, 1e-8) (ATen's clamp of
 * cosine_similarity) in an OPAQUE layout -- the operand order of the search kernel's matrix instruction, D padded to a multiple of 8, documents
 * in groups of 32.  The address of a document depends on its number and D alone, never on the capacity: an index grows by copying its bytes
 * into a larger buffer.  nir_retrieve_index_bytes: the size of that buffer (0 for arguments outside the envelope); 256-byte alignment is required.
 *
 * nir_retrieve_add: documents offset .. offset + m - 1 := the unit rows of reps [m, D] (raw tower outputs).  A row with a non-finite component
 * is stored as zeros and ORs bit 0 into *err_flag (may be NULL).  Rows are independent: any split of a corpus into calls gives the same bytes.
 * nir_retrieve_export / nir_retrieve_import: the stored unit rows offset .. offset + m - 1 to / from plain [m, D] order, bit for bit (no
 * normalisation) -- how an index is saved without its layout.
 * ------------------------------------------------------------------------------------------------ */
size_t nir_retrieve_index_bytes(int64_t capacity, int D);
int nir_retrieve_add(const float* reps, int64_t m, int D, void* index, int64_t capacity, int64_t offset, int32_t* err_flag, nir_stream_t stream);
int nir_retrieve_export(const void* index, int64_t capacity, int D, int64_t offset, int64_t m, float* rows, nir_stream_t stream);
int nir_retrieve_import(const float* rows, int64_t m, int D, void* index, int64_t capacity, int64_t offset, nir_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Per query b of queries [B, D] (raw tower outputs, normalised like the documents; a non-finite row counts as zeros and ORs bit 1 into
 * *err_flag) the k largest s[b, j] = q^_b . d^_j over the documents j < M of the index: top_val [B, k] fp32 in descending order, top_idx [B, k]
 * int32, the smaller document first among equal values; slots beyond M hold -inf / -1.  1 <= k <= NIR_RETRIEVE_MAX_K, 0 <= M < 2^31,
 * 0 <= B < 2^31.  The D-sum of a pair runs in one fixed order on the fp32 matrix pipe, so the bits of s[b, j] do not depend on B, M, k, the
 * form or the document's position, and exact duplicates tie bit for bit.  All index addressing is 64-bit.
 * Fused (the default): one workgroup per (tile of 32 or 64 queries, chunk of nir_retrieve_chunk_docs() documents) keeps a sorted list of k
 * entries per query on chip; the workspace holds the chunks' lists, which nir_retrieve_merge's kernel merges.  No B x M score buffer exists.
 * Plain: the same score tiles written to a score matrix in the workspace -- stored [M, B], document-major -- and the same selection reading it back.
 * ------------------------------------------------------------------------------------------------ */
size_t nir_retrieve_topk_workspace_bytes(int64_t B, int64_t M, int D, int k, int form);
int nir_retrieve_topk(const float* queries, int64_t B, const void* index, int64_t M, int D, int k, int form, void* workspace,
                      size_t workspace_bytes, int32_t* err_flag, float* top_val, int32_t* top_idx, nir_stream_t stream);

/* The merge of P sorted partial lists vals / idx [P, B, k] (descending, the smaller index first among equal values, unused slots -inf / -1)
 * into out_val / out_idx [B, k] under the same rule: one wave per query.  A sharded index is an all-gather of the shards' lists plus this call
 * (with the shards' document offsets added to idx).  1 <= P < 2^20. */
int nir_retrieve_merge(const float* vals, const int32_t* idx, int P, int64_t B, int k, float* out_val, int32_t* out_idx, nir_stream_t stream);

/* The number of documents one workgroup of the search walks: chunk c covers documents c C .. (c + 1) C - 1. */
int nir_retrieve_chunk_docs(void);

#ifdef __cplusplus
}
#endif

#endif
