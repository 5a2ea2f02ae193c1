// The row sources of the generator kernels that take one (csrc/beam.hip: beam_gen_topk_kernel; csrc/score.hip: score_gen_target_kernel): where a
// workgroup's decode rows come from and how the grid maps to (row block, vocabulary range).  The kernel stages its NR = 16 NBT rows from b0 on
// into the LDS planes [2 terms][NR][K + 8] in K/4 chunks a row: load() reads chunk c of a row, store() puts it into the planes.  map() reads
// blockIdx of a grid of nvr ranges x ceil(R / NR) row blocks.
#pragma once
#include "split2.hpp"

namespace nir {

struct BeamRowsF32 {                                  // fp32 rows x [Bd, K], split into the two fp16 terms on load; a row block's ranges are adjacent
    using elem = float;
    template <int NR>
    static __device__ __forceinline__ void map(int nvr, int64_t, int& vr, int64_t& b0) {
        vr = (int)(blockIdx.x % nvr);
        b0 = (int64_t)(blockIdx.x / nvr) * NR;
    }
    using chunk = float4;                             // four fp32 of a row -> four fp16 in either plane
    static __device__ __forceinline__ float4 load(const float* __restrict__ x, int64_t row, int c, int K) {
        return *reinterpret_cast<const float4*>(x + row * K + c * 4);
    }
    template <int NR>
    static __device__ __forceinline__ void store(_Float16* sm, int r, int c, int LD, float4 v) {
        const Split2x4 sp = split2(v);
        _Float16* d = sm + r * LD + c * 4;
        *reinterpret_cast<uint2*>(d) = sp.hi;
        *reinterpret_cast<uint2*>(d + NR * LD) = sp.lo;
    }
};
// The rows as the folded LSTM step writes them, h16 [row][K/8][2 terms][8] (HredQS): one 16-byte copy per (row, k-group,
// term), no fp32 load, no conversion.  The grid is hq_gen_argmax_kernel's nrb row blocks x nvr ranges with its blockIdx mapping: the row blocks
// of a range run together on one XCD and share its L2 (nvr a multiple of 8), else they are adjacent in dispatch order.  A beam has W times the
// rows of the greedy decode, so a range is read by W times the row blocks.
struct BeamRowsSplit {
    using elem = _Float16;
    template <int NR>
    static __device__ __forceinline__ void map(int nvr, int64_t R, int& vr, int64_t& b0) {
        const int nrb = (int)((uint64_t)(R + NR - 1) / NR);                       // the launcher's row-block count
        int rb;
        if (nvr % 8 == 0) {
            const int j = (int)(blockIdx.x >> 3);
            rb = j % nrb;
            vr = (j / nrb) * 8 + (int)(blockIdx.x & 7);
        } else {
            rb = (int)(blockIdx.x % nrb);
            vr = (int)(blockIdx.x / nrb);
        }
        b0 = (int64_t)rb * NR;
    }
    using chunk = uint4;                              // the eight fp16 of one (k-group, term): 16 bytes, copied
    static __device__ __forceinline__ uint4 load(const _Float16* __restrict__ h16, int64_t row, int c, int K) {
        return *reinterpret_cast<const uint4*>(h16 + (row * (K / 4) + c) * 8);
    }
    template <int NR>
    static __device__ __forceinline__ void store(_Float16* sm, int r, int c, int LD, uint4 v) {
        *reinterpret_cast<uint4*>(sm + (c & 1) * NR * LD + r * LD + (c >> 1) * 8) = v;
    }
};

}  // namespace nir
