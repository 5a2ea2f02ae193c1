// Shared by the greedy decoders (csrc/cars_decode.hip, csrc/seq2seq.hip): the GEMM launchers of gemm.hip and the small launches every
// decoder makes between its steps.  The kernels live in cars_decode.hip; these are their host-side launchers.
#pragma once
#include "split2.hpp"

namespace nir {

int launch_linear(const float* a, int64_t lda, const int64_t* ids, const float* table, int E, int64_t rows_per_seq,
                  int64_t seq_stride, const float* w, int64_t ldw, const float* bias, const float* bias2, float* c,
                  int64_t ldc, int64_t M, int N, int K, int act, hipStream_t st);

// p[i] = v, i < n
int launch_fill_i64(int64_t* p, int64_t v, int64_t n, hipStream_t st);
// h [n = rows * H] fp32 -> the fp16 term pairs of the fp16-term LSTM step: [row][H/8][2 terms][8]  (H % 8 == 0)
int launch_h16_pack(const float* h, int64_t n, _Float16* out, hipStream_t st);
// pred[i * pstride] = argmax_v logits[i, v] (first index on ties); tgt[i] = lut ? lut[pred] : pred, <unk> (1) outside [0, Vsrc)
int launch_argmax_map(const float* logits, int64_t V, const int64_t* lut, int64_t* pred, int64_t pstride, int64_t* tgt, int64_t Vsrc, int64_t Bd,
                      hipStream_t st);
// the same from `nparts` partial (value, index) pairs per row, pval / pidx [nparts][Bd]
int launch_argmax_finish(const float* pval, const int* pidx, int nparts, int64_t Bd, const int64_t* lut, int64_t* pred, int64_t pstride, int64_t* tgt,
                         int64_t Vsrc, hipStream_t st);
// multiProcessorCount of the current device (256 if unknown)
int device_cu_count();

}  // namespace nir
