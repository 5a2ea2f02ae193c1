/* libneuroir_hip: the GRU decoders of Seq2seq and ACG.  Included by neuroir_hip.h (which defines the types used here); not meant to be
 * included on its own. */
#ifndef NEUROIR_GRU_DECODE_H
#define NEUROIR_GRU_DECODE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * GRU decoders of Seq2seq and ACG (rnn_type 'GRU': neuroir/decoders/decoder.py:175-177 builds the decoder's state from the encoder's single
 * h_n, decoders/rnn_decoder.py:46-47 runs torch.nn.GRU on it).  csrc/gru_step.hip.  Gate order r, z, n;
 *   r = sigma(W_ir x + b_ir + W_hr h + b_hr), z = sigma(W_iz x + b_iz + W_hz h + b_hz), n = tanh(W_in x + b_in + r (W_hn h + b_hn)),
 *   h' = (1 - z) n + z h.
 * ------------------------------------------------------------------------------------------------ */
/* weight_hh_l0 [3H,H] -> two fp16 term planes (w = w1 + 2^-11 w2') in MFMA A-fragment order [H/16 unit groups][3 gates][H/32][2 terms][64 lanes][8].
 * H a positive multiple of 32 (bytes() returns 0 otherwise).  err_flag (int, may be NULL) gets bit 1 (value 2) when a weight is outside the
 * split's range (|w| >= 2^15 or not finite): the caller then leaves the fragment out and the plain step runs. */
size_t nir_gru_step_whh_frag_bytes(int H);
int nir_gru_step_pack_whh_frag(const float* w_hh, int H, void* frag, int* err_flag, nir_stream_t stream);
/* ONE decoder step (rnn_decoder.py:46-47 for a single time step) for B rows: x[b] = table[ids[b]] (ids outside [0, V) read row 1, <unk>),
 * h_next [B,H] = GRU(x, h_prev).  The input side is either gate_fold [V,3H] = table W_ih^T + b_ih + (b_hr, b_hz, 0) (nir_linear_f32 over the
 * table with the combined bias; b_hn is NOT folded) or, gate_fold NULL, table [V,E] with w_ih [3H,E] and b_ih.  w_hh [3H,H], b_hh [3H].
 * Fast form -- whh_frag given, H % 32 == 0, tunable exact_f32 off: the recurrent product runs as three v_mfma_f32_16x16x32_f16 per 32-wide
 * k-block over fp16 term pairs, the cell in the same kernel (one launch with gate_fold; the gathered input GEMM in front of it without).
 * h16_prev (optional): h_prev as term pairs [B][H/8][2 terms][8] as a previous call wrote them to h16_next; built from h_prev when NULL.
 * Plain form -- everything else, H % 4 == 0: exact fp32 (two GEMMs and the cell kernel).  h16_next (optional, H % 8 == 0) gets the term pairs
 * of h_next in either form.  h_next must not alias h_prev.  Enqueued on `stream`; never synchronises, allocates nothing; the same inputs give
 * the same bits.  Bad arguments: NIR_ERR_BAD_ARG, nothing enqueued.  B == 0: nothing enqueued. */
size_t nir_gru_step_workspace_bytes(int64_t B, int H);
int nir_gru_step(const int64_t* ids, int64_t B, const float* table, int64_t V, int E, const float* w_ih, const float* b_ih, const float* gate_fold,
                 const float* w_hh, const float* b_hh, const void* whh_frag, int H, const float* h_prev, const void* h16_prev, float* h_next,
                 void* h16_next, void* workspace, size_t workspace_bytes, nir_stream_t stream);
/* nir_seq2seq_decode_greedy / nir_acg_decode_greedy with the GRU step (seq2seq.py:118-195 with rnn_type 'GRU'): no cell state.  The struct is
 * nir_seq2seq_decoder_weights with rnn_* read as [3H,E], [3H,H], [3H]; rnn_gate_fold [V,3H] and rnn_whh_frag the forms above (both or
 * neither).  The same house rules. */
size_t nir_seq2seq_gru_decode_workspace_bytes(int64_t B, int QL, const nir_seq2seq_decoder_weights* w /*host*/);
int nir_seq2seq_gru_decode_greedy(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, const float* table,
                                  int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w /*host*/,
                                  void* workspace, size_t workspace_bytes, int64_t* predictions, float* attentions, nir_stream_t stream);
size_t nir_acg_gru_decode_workspace_bytes(int64_t B, int QL, int CV, const nir_seq2seq_decoder_weights* w /*host*/,
                                          const nir_acg_copy_weights* cw /*host*/);
int nir_acg_gru_decode_greedy(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, const float* table,
                              int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w /*host*/,
                              const nir_acg_copy_weights* cw /*host*/, const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src,
                              int CV, void* workspace, size_t workspace_bytes, int64_t* predictions, float* attentions, nir_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
