// Shared by the split-fp16 conv + pool kernels (arci.hip: 1-D, arcii.hip: 2-D): the tile shape, the staging helpers, the packed-weight
// entry and the 1-D launch, which ARC-II's first stage runs as it is.
#pragma once
#include "split2.hpp"

namespace nir {

constexpr int CV_ROWS = 64;        // conv positions per workgroup (4 MFMA row tiles)
constexpr int CV_COLS = 128;       // filters per workgroup: 4 waves x 2 column tiles of 16
constexpr int CV_CT = 2, CV_RT = 4;
constexpr int CV_EP_LD = CV_COLS + 4;
constexpr int CV_MAX_C = 1024, CV_MAX_F = 1024, CV_MAX_K = 7, CV_MAX_P = CV_ROWS;

struct ConvSide {
    const int64_t* ids;       // [M, L] token ids (x is then the table [V, C]) or NULL (x is the dense [M, L, C] activation)
    const float* x;
    const uint4* planes;      // conv1d_pack_kernel's fragments
    const float* wt;          // fp32 [k C][F]
    const float* bias;
    const float* head_w;      // NULL: out is [M, L / p, F]; else w_eff [F][L / p] and out is the partial list [M L/p][NCB][2]
    float* out;
    int64_t M;
    int L;
};
struct ConvArgs {
    ConvSide s[2];
    int64_t nblk0;            // blocks [0, nblk0) belong to s[0], the rest to s[1]
    int C, F, k, p, act;
};

__device__ __forceinline__ void cv_load8(const float* src, int c, int C, bool vec4, float (&v)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (!src) return;
    if (vec4) {                                  // C % 4 == 0: rows are 16-byte aligned and a float4 is inside the row or outside it
        if (c + 4 <= C) {
            const float4 q = *reinterpret_cast<const float4*>(src + c);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        }
        if (c + 8 <= C) {
            const float4 q = *reinterpret_cast<const float4*>(src + c + 4);
            v[4] = q.x, v[5] = q.y, v[6] = q.z, v[7] = q.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (c + e < C) v[e] = src[c + e];
    }
}

// LDS slot (16 bytes = 8 halfs) of (buffer, term, row, 8-channel chunk).  The chunk is rotated by the row's group of four so that the
// ds_read_b128 of an A fragment (lane l: row l & 15, chunk l >> 4) meets 16 different bank quads in each of its lane groups.
__device__ __forceinline__ int cv_slot(int buf, int term, int row, int chunk) {
    return ((buf * 2 + term) * CV_ROWS + row) * 4 + (chunk ^ ((0 - (row >> 2)) & 3));
}

inline size_t conv_ncb(int F) { return (size_t)((F + CV_COLS - 1) / CV_COLS); }

// arci.hip
int conv_check(const nir_conv1d_layer* ly, const char* who);
int conv_launch(ConvSide s0, ConvSide s1, int C, int F, int k, int p, int act, int path, hipStream_t st, const char* who);
ConvSide conv_side(const int64_t* ids, const float* x, const nir_conv1d_layer* ly, const float* head_w, float* out, int64_t M, int L);
// weight [F][C][taps] -> fragments over the tap-major K order taps * roundup(C, 32), and the fp32 transpose [taps C][F]; no limit checks
int conv_pack_launch(const float* w, int C, int F, int taps, void* planes, float* wt, int* flag, hipStream_t st, const char* who);

}  // namespace nir
