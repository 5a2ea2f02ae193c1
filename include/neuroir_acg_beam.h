/* libneuroir_hip: beam search for ACG, the Seq2seq recommender with a copy generator (LSTM and GRU decoders).  Included by neuroir_hip.h (which
 * defines the types used here); not meant to be included on its own.  csrc/beam.hip. */
#ifndef NEUROIR_ACG_BEAM_H
#define NEUROIR_ACG_BEAM_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * The reference ships no search; the semantics are this project's and extend those of neuroir_beam.h in everything not
 * restated here: row layout row = k B + b, step 0 with beam 0 alone live, the frozen (k, EOS) offer of a finished beam, max_len steps with no
 * early stop, fixed shapes, no host synchronisation, 1 <= W <= NIR_BEAM_MAX_W, VT >= W.
 * Per live beam row r = k B + b, with the quantities of nir_acg_gen_select in its fp32 expressions -- l = W_g o + b_g (l[PAD] := -1e-20 behind
 * the linear), m = max l, Z = sum exp(l - m), z = sigmoid(x), 1 - z = sigmoid(-x), mass[c] = z sum_{j < len[b], map[b, j] = c} a[r, j]
 * (j ascending) -- the candidates are, by EXTENDED id e in [0, VT + CV):
 *   a target word v < VT that no slot collapses onto     P = (1 - z) exp(l[v] - m) / Z
 *   a target word t that one or more slots c >= 2 collapse onto, offered ONCE
 *                                                         P = (1 - z) exp(l[t] - m) / Z + the sum of those slots' mass
 *   a slot VT + c that is not collapsed                   P = mass[c]
 *   a collapsed slot                                      NOT a candidate.  The reference leaves 1e-10 there; its word is already offered as
 *                                                         t, and offering it again would put the same word twice into an n-best list.
 * The copy maps src_map_idx [B, QL], ext2tgt [B, CV], ext2src [B, CV] and source_len [B] are NOT repeated: beam row r reads source row r % B.
 *   offers   cum[b, k] + logf(P); P = 0 gives -inf, which loses to every finite score and never stalls the selection.
 *   select   score descending, ties to the smaller flat index k (VT + CV) + e.
 *   finished e == NIR_BEAM_EOS.
 *   feedback tgt2src[e] (e itself without a table) below VT, ext2src[b, e - VT] from VT on; <unk> (1) outside [0, V).
 * The W best of a row lie among at most W + CV candidates: every collapse target and every slot is evaluated exactly, and a word that is no
 * target and lies outside the row's raw top-W logits (PAD substituted) is dominated by all W entries of that list.
 * House rules of every entry: enqueued on `stream`; never synchronises, allocates nothing; the same inputs give the same bits; bad arguments
 * (W outside 1..8, VT < W, QL outside [1, 4096], CV outside [2, 1024], null pointers) return NIR_ERR_BAD_ARG and a short workspace
 * NIR_ERR_WORKSPACE, with nothing enqueued.
 * ------------------------------------------------------------------------------------------------ */

/* The two per-row launches: per decode row r (of `rows`, reading source row r % nsrc) the W best (log P, extended id) of the collapsed
 * extended distribution, descending, the smaller id first among equals.  o [rows, K]: attentional outputs; copy_attn row r at copy_attn +
 * r * attn_stride, [QL]; source_len [nsrc], src_map_idx [nsrc, QL], ext2tgt / ext2src [nsrc, CV] (ext2src is not read here: the selection
 * feeds back through it); top_val [rows, W] fp32, top_idx [rows, W] int32.  Fused form -- gen_frag given (nir_seq2seq_pack_gen_frag), K a
 * multiple of 32 in [32, 1024], tunable exact_f32 off: the PAD-substituting generator top-k, the logits never leave the chip.  Plain form
 * otherwise (K % 4 == 0): the fp32 GEMM into the workspace and one workgroup per row.  rows == 0: nothing enqueued. */
size_t nir_acg_beam_gen_select_workspace_bytes(int64_t rows, int K, int64_t VT, int W, int fused);
int nir_acg_beam_gen_select(const float* o, int64_t rows, int64_t nsrc, int K, const float* gen_w, const float* gen_b, const void* gen_frag,
                            int64_t VT, int W, const float* copy_w, const float* copy_b, const float* copy_attn, int64_t attn_stride,
                            const int64_t* source_len, int QL, const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src, int CV,
                            void* workspace, size_t workspace_bytes, float* top_val, int32_t* top_idx, nir_stream_t stream);

/* nir_beam_select over extended ids: top_val = log P and lse = NULL (read as 0) behind the entry above; token [B, W] are EXTENDED ids, and
 * next_ids go through tgt2src below VT and ext2src [B, CV] from VT on. */
int nir_acg_beam_select(const float* top_val, const int32_t* top_idx, const float* lse, int64_t B, int W, int64_t VT, int CV, const int64_t* tgt2src,
                        const int64_t* ext2src, int64_t V, float* cum, int32_t* finished, int32_t* backptr, int32_t* token, int64_t* next_ids,
                        nir_stream_t stream);

/* The whole search: the arguments of nir_acg_decode_greedy plus W.  dec_h, dec_c [B W, H]: the initial state repeated in the layout above;
 * memory_bank, source_len and the three maps are NOT repeated.  Outputs, all backtracked, best beam first: predictions [B, W, max_len] int64
 * (EXTENDED ids, EOS repeated after the first EOS), scores [B, W] fp32, lengths [B, W] int64, attentions [B, W, max_len, QL] fp32 (the
 * decoder's own attention, as in the greedy decode), backptr (optional) [max_len, B, W] int32.  B == 0: nothing enqueued, in every form. */
size_t nir_acg_beam_decode_workspace_bytes(int64_t B, int QL, int CV, int W, int max_len, const nir_seq2seq_decoder_weights* w /*host*/,
                                           const nir_acg_copy_weights* cw /*host*/);
int nir_acg_beam_decode(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL,
                        const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                        const nir_seq2seq_decoder_weights* w /*host*/, const nir_acg_copy_weights* cw /*host*/, const int64_t* src_map_idx,
                        const int64_t* ext2tgt, const int64_t* ext2src, int CV, int W, void* workspace, size_t workspace_bytes, int64_t* predictions,
                        float* scores, int64_t* lengths, float* attentions, int32_t* backptr, nir_stream_t stream);
/* The same with the GRU decoder (no cell state). */
size_t nir_acg_beam_gru_decode_workspace_bytes(int64_t B, int QL, int CV, int W, int max_len, const nir_seq2seq_decoder_weights* w /*host*/,
                                               const nir_acg_copy_weights* cw /*host*/);
int nir_acg_beam_gru_decode(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, const float* table, int64_t V,
                            int E, const int64_t* tgt2src, int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w /*host*/,
                            const nir_acg_copy_weights* cw /*host*/, const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src, int CV,
                            int W, void* workspace, size_t workspace_bytes, int64_t* predictions, float* scores, int64_t* lengths, float* attentions,
                            int32_t* backptr, nir_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
