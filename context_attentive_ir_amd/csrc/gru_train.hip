// Train-mode GRU (neuroir/encoders/rnn_encoder.py:62-141 with rnn_type = 'GRU' under models/ranker.py:192-230; torch.nn.GRU, gate order r, z, n):
//
//   nir_gru_train_fwd       recurrence for H <= 128 per direction that also stores (r, z, n, q = W_hn h + b_hn) of every valid step (one thread per gate
//                           row, W_hh in registers)
//   nir_gru_train_bwd       BPTT: dgx (gradient of the input-side gate pre-activations) and dq (gradient of q) of every step; W_hh resident on the
//                           fp32 matrix cores (gru_train_bwd_mfma_kernel) or the VALU form (gru_train_bwd_kernel)
//   nir_gru_cell_seq_fwd / _bwd   the cell inside [B,T,.] sequence buffers, any H (autograd._GRUSeq: recurrent products stay on nir_linear_f32)
//
//   r = sigma(gx_r + gh_r)   z = sigma(gx_z + gh_z)   q = gh_n   n = tanh(gx_n + r q)   h_t = (1 - z) n + z h_{t-1}      gh = h_{t-1} W_hh^T + b_hh
//   dn = dh (1 - z)   dz = dh (h_{t-1} - n)   da_n = dn (1 - n^2)   da_r = da_n q r (1 - r)   da_z = dz z (1 - z)   dq = da_n r
//   dgx = (da_r, da_z, da_n)   dgh = (da_r, da_z, dq)   dh_{t-1} = z dh + dgh W_hh
//
// dgx and dgh differ in the n slot only, so the kernels write dgx [M,T,ND*3H] and dq [M,T,ND*H] (4 floats per cell instead of 6): dW_hh's r / z
// rows are reduced from dgx, its n rows from dq (autograd._BiGRU.backward).  Packed-sequence semantics: steps at t >= length do not run, out and
// every gradient are zero there, the reverse direction starts at t = length - 1 from the zero state.  No float atomics: same inputs, same bits.
#include "split2.hpp"

namespace nir {

constexpr int GSQ = 4;           // sequences per workgroup of the one-thread-per-gate-row kernels

__device__ __forceinline__ int clamp_len(const int64_t* lens, int64_t m, int64_t M, int T) {
    if (m >= M) return 0;
    const int64_t l = lens ? lens[m] : (int64_t)T;
    return l < 0 ? 0 : (l > T ? T : (int)l);
}

// ---------------------------------------------------------------------------------------------------------------------
// Forward.  One workgroup = GSQ
// sequences of one direction, one thread per gate row j < 3H (<= 384 threads): its W_hh row lives in registers,
// h_{t-1} of the GSQ sequences in LDS (the layout of lstm_train_fwd_kernel).  Phase 1: every thread forms gh_j; the r / z rows add gx and apply
// the sigmoid, the n rows hand q to LDS.  Phase 2: thread j < H owns unit j -- n, h_t, the four stored activations.
// ---------------------------------------------------------------------------------------------------------------------
struct GruTrainArgs {
    const float* gin;      // [M,T,ND*3H]  x W_ih^T + b_ih
    const int64_t* lens;
    const float* whh;      // [ND,3H,H]
    const float* bhh;      // [ND,3H]
    float* out;            // [M,T,ND*H]
    float* act;            // [M,T,ND,4H]  (r, z, n, q)
    float* hn;             // [ND,M,H] or NULL
    int64_t M;
    int T, H, ND;
};

template <int HP>
__global__ __launch_bounds__(384) void gru_train_fwd_kernel(GruTrainArgs p) {
    extern __shared__ float sm[];
    float* hs = sm;                       // [GSQ][H]
    float* gs = sm + GSQ * p.H;           // [GSQ][3H]: sigma(r), sigma(z), q
    const int j = threadIdx.x, H = p.H, H3 = 3 * H, T = p.T;
    const int dir = blockIdx.y;
    const int64_t m0 = (int64_t)blockIdx.x * GSQ;
    const bool jv = j < H3;
    float w[HP];
#pragma unroll
    for (int k = 0; k < HP; ++k) w[k] = (jv && k < H) ? p.whh[((int64_t)dir * H3 + j) * H + k] : 0.f;
    const float bj = jv ? p.bhh[(int64_t)dir * H3 + j] : 0.f;
    int len[GSQ];
    int tmax = 0;
#pragma unroll
    for (int s = 0; s < GSQ; ++s) {
        len[s] = clamp_len(p.lens, m0 + s, p.M, T);
        tmax = max(tmax, len[s]);
        if (j < H) hs[s * H + j] = 0.f;
    }
    __syncthreads();
    const int gate = jv ? j / H : 0;
    const int64_t ldg = (int64_t)p.ND * H3;
    for (int step = 0; step < tmax; ++step) {
#pragma unroll
        for (int s = 0; s < GSQ; ++s) {
            if (step < len[s] && jv) {
                const int t = dir == 0 ? step : len[s] - 1 - step;
                const float* hv = hs + s * H;
                float a = bj;
#pragma unroll
                for (int k = 0; k < HP; ++k)
                    if (k < H) a = fmaf(w[k], hv[k], a);
                if (gate < 2) {
                    a += p.gin[((m0 + s) * T + t) * ldg + dir * H3 + j];
                    a = 1.0f / (1.0f + expf(-a));
                }
                gs[s * H3 + j] = a;
            }
        }
        __syncthreads();
        if (j < H) {
#pragma unroll
            for (int s = 0; s < GSQ; ++s) {
                if (step < len[s]) {
                    const int t = dir == 0 ? step : len[s] - 1 - step;
                    const int64_t row = (m0 + s) * T + t;
                    const float r = gs[s * H3 + j], z = gs[s * H3 + H + j], q = gs[s * H3 + 2 * H + j];
                    const float n = tanhf(p.gin[row * ldg + dir * H3 + 2 * H + j] + r * q);
                    const float h = (1.f - z) * n + z * hs[s * H + j];
                    hs[s * H + j] = h;
                    p.out[row * (int64_t)(p.ND * H) + dir * H + j] = h;
                    float* a = p.act + (row * p.ND + dir) * (int64_t)(4 * H);
                    a[j] = r; a[H + j] = z; a[2 * H + j] = n; a[3 * H + j] = q;
                }
            }
        }
        __syncthreads();
    }
    if (j < H) {
#pragma unroll
        for (int s = 0; s < GSQ; ++s) {
            if (m0 + s < p.M) {
                for (int t = len[s]; t < T; ++t) p.out[((m0 + s) * T + t) * (int64_t)(p.ND * H) + dir * H + j] = 0.f;
                if (p.hn) p.hn[((int64_t)dir * p.M + m0 + s) * H + j] = hs[s * H + j];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// BPTT, VALU form (every shape; the dispatcher keeps it for the hidden sizes the matrix-core form does not take).  Thread j < H owns unit j of
// the GSQ sequences: gate gradients, the direct z dh path in a register.  dh_{t-1} = dgh_t W_hh: thread (g = j / H, k = j % H) sums the rows
// [g H, (g+1) H) of column k (coalesced reads of W_hh rows from L2), the three partial sums meet in LDS.
// ---------------------------------------------------------------------------------------------------------------------
struct GruBwdArgs {
    const float* dout;     // [M,T,ND*H]
    const float* dhn;      // [ND,M,H] or NULL
    const float* act;      // [M,T,ND,4H]
    const float* out;      // [M,T,ND*H]: h_{t-1} is the row before (forward) / after (reverse) the step's row, zero at a sequence's first step
    const int64_t* lens;
    const float* whh;
    float* dgx;            // [M,T,ND*3H]
    float* dq;             // [M,T,ND*H]
    int64_t M;
    int T, H, ND;
};

__global__ __launch_bounds__(384) void gru_train_bwd_kernel(GruBwdArgs p) {
    extern __shared__ float sm[];
    const int H = p.H, H3 = 3 * H, T = p.T;
    float* dg = sm;                       // [GSQ][3H] dgh of the current step
    float* dhr = dg + GSQ * H3;           // [GSQ][H]  carried dh
    float* part = dhr + GSQ * H;          // [3][GSQ][H]
    const int j = threadIdx.x;
    const int dir = blockIdx.y;
    const int64_t m0 = (int64_t)blockIdx.x * GSQ;
    const bool jv = j < H3;
    const int g = jv ? j / H : 0, k = jv ? j % H : 0;
    int len[GSQ];
    int tmax = 0;
    float dhd[GSQ];
#pragma unroll
    for (int s = 0; s < GSQ; ++s) {
        len[s] = clamp_len(p.lens, m0 + s, p.M, T);
        tmax = max(tmax, len[s]);
        dhd[s] = 0.f;
        if (j < H) dhr[s * H + j] = (m0 + s < p.M && p.dhn) ? p.dhn[((int64_t)dir * p.M + m0 + s) * H + j] : 0.f;
    }
    __syncthreads();
    const int64_t ldo = (int64_t)p.ND * H;
    for (int step = tmax - 1; step >= 0; --step) {
        if (j < H) {
#pragma unroll
            for (int s = 0; s < GSQ; ++s) {
                float ar = 0.f, az = 0.f, aq = 0.f;
                if (step < len[s]) {
                    const int t = dir == 0 ? step : len[s] - 1 - step;
                    const int64_t row = (m0 + s) * T + t;
                    const float* a = p.act + (row * p.ND + dir) * (int64_t)(4 * H);
                    const float r = a[j], z = a[H + j], n = a[2 * H + j], q = a[3 * H + j];
                    const float hprev = step > 0 ? p.out[(row + (dir == 0 ? -1 : 1)) * ldo + dir * H + j] : 0.f;
                    const float dh = p.dout[row * ldo + dir * H + j] + dhr[s * H + j];
                    const float dan = dh * (1.f - z) * (1.f - n * n);
                    ar = dan * q * r * (1.f - r);
                    az = dh * (hprev - n) * z * (1.f - z);
                    aq = dan * r;
                    dhd[s] = dh * z;
                    float* o = p.dgx + row * (int64_t)(p.ND * H3) + dir * H3;
                    o[j] = ar; o[H + j] = az; o[2 * H + j] = dan;
                    p.dq[row * ldo + dir * H + j] = aq;
                }
                dg[s * H3 + j] = ar; dg[s * H3 + H + j] = az; dg[s * H3 + 2 * H + j] = aq;
            }
        }
        __syncthreads();
        if (jv) {
            float a[GSQ];
#pragma unroll
            for (int s = 0; s < GSQ; ++s) a[s] = 0.f;
            const float* wp = p.whh + ((int64_t)dir * H3 + g * H) * H + k;
            for (int jj = 0; jj < H; ++jj) {
                const float wv = wp[(int64_t)jj * H];
#pragma unroll
                for (int s = 0; s < GSQ; ++s) a[s] = fmaf(dg[s * H3 + g * H + jj], wv, a[s]);
            }
#pragma unroll
            for (int s = 0; s < GSQ; ++s) part[(g * GSQ + s) * H + k] = a[s];
        }
        __syncthreads();
        if (j < H) {
#pragma unroll
            for (int s = 0; s < GSQ; ++s)
                if (step < len[s])    // sequences that have not started yet (step >= len) keep the final-state gradient
                    dhr[s * H + j] = dhd[s] + ((part[(0 * GSQ + s) * H + j] + part[(1 * GSQ + s) * H + j]) + part[(2 * GSQ + s) * H + j]);
        }
        __syncthreads();
    }
    if (j < H) {
#pragma unroll
        for (int s = 0; s < GSQ; ++s) {
            if (m0 + s < p.M) {
                for (int t = len[s]; t < T; ++t) {
                    const int64_t row = (m0 + s) * T + t;
                    float* o = p.dgx + row * (int64_t)(p.ND * H3) + dir * H3;
                    o[j] = 0.f; o[H + j] = 0.f; o[2 * H + j] = 0.f;
                    p.dq[row * ldo + dir * H + j] = 0.f;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// BPTT on the matrix cores with W_hh RESIDENT, in the structure of lstm_train_bwd_mfma_kernel (csrc/train.hip): 16 sequences x one direction per
// workgroup, one wave per 16-unit tile (HP / 16 rounded up: 2 .. 8 waves),
//     dh_{t-1}[unit, seq] = z dh + sum_jj W_hh[jj, unit] * dgh_t[seq, jj]     as   D[16 units x 16 seqs] += A[16 units x 4] B[4 x 16 seqs]
// on v_mfma_f32_16x16x4_f32 (exact fp32), the reduction over (gate, unit) = 3 x HP values (HP = H rounded up to 4): 3 HP / 4 k-steps per step,
// padded to a multiple of four (the B operand is read 16 bytes = four k-steps at a time; the padding's A fragments are zero).  Fragment lane
// (unit = lane & 15, kq = lane >> 4) holds W_hh[g H + 4 c + kq][unit] for k-step (g, c) in registers for all T steps.  The C/D layout hands a lane
// (seq = lane & 15, units 4 (lane >> 4) + r): the lane that receives dh_{t-1} of a cell computes that cell's gate gradients in the next step and
// adds the z dh term it kept in a register -- dh never leaves registers.  Per step: gate gradients of the lane's 4 cells (act row, h_{t-1} row and
// dout row prefetched one step ahead) -> dgx / dq to HBM and dgh, as the B operand, to LDS [seq][kq][k-step] -> one LDS barrier -> the MFMAs on
// two accumulator chains (one chain is latency-bound at 40 against 32 cycles with a single wave per SIMD).  Two LDS buffers, one barrier per step.
// ---------------------------------------------------------------------------------------------------------------------
template <int HP>
__global__ __launch_bounds__(64 * ((HP + 15) / 16), 1) void gru_train_bwd_mfma_kernel(GruBwdArgs p) {
    constexpr int SEQ = 16, NWV = (HP + 15) / 16, NTH = 64 * NWV;
    constexpr int KG = HP / 4;                             // k-steps per gate
    constexpr int NKS = (3 * KG + 3) / 4 * 4;
    constexpr int RS = NKS + 4;                            // LDS row stride in floats (the padding lstm_train_bwd_mfma_kernel measured)
    extern __shared__ __attribute__((aligned(16))) float smb[];
    float* dgs = smb;                                      // [2][SEQ][4][RS]
    int* lens_s = reinterpret_cast<int*>(smb + 2 * SEQ * 4 * RS);
    const int H = p.H, H3 = 3 * H, H4 = 4 * H, T = p.T, ND = p.ND;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sq = lane & 15, pq = lane >> 4;
    const int dir = blockIdx.y;
    const int64_t m0 = (int64_t)blockIdx.x * SEQ;
    const bool sv = m0 + sq < p.M;
    if (tid < SEQ) lens_s[tid] = clamp_len(p.lens, m0 + tid, p.M, T);
    for (int e = tid; e < 2 * SEQ * 4 * RS; e += NTH) dgs[e] = 0.f;
    __syncthreads();
    int tmax = 0;
#pragma unroll
    for (int s2 = 0; s2 < SEQ; ++s2) tmax = max(tmax, lens_s[s2]);
    const int len = lens_s[sq];
    // A fragments: output unit uo = 16 wave + (lane & 15); k-step ks = g KG + c reads W_hh[g H + 4 c + pq][uo] (unconditional loads from clamped
    // indices, masked by a multiply: see lstm_train_bwd_mfma_kernel)
    float afr[NKS];
    {
        const int uo = 16 * wave + sq;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            if (ks < 3 * KG) {
                const int g = ks / KG, c = ks % KG, ui = 4 * c + pq;
                afr[ks] = p.whh[((int64_t)dir * H3 + (int64_t)g * H + (ui < H ? ui : H - 1)) * H + (uo < H ? uo : H - 1)] * ((uo < H && ui < H) ? 1.f : 0.f);
            } else {
                afr[ks] = 0.f;
            }
        }
    }
    const int ub = 16 * wave + 4 * pq;                      // the lane's cells: sequence sq, units ub + r
    const int64_t mrow = sv ? m0 + sq : m0;                 // (idle lanes read a valid row and are masked)
    const int64_t ldo = (int64_t)ND * H;
    float dh[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int u = ub + r;
        dh[r] = (sv && u < H && p.dhn) ? p.dhn[((int64_t)dir * p.M + m0 + sq) * H + u] : 0.f;
    }
    struct CellIn { float a[4][4]; float hp[4], dy[4]; };
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(p.act) | reinterpret_cast<uintptr_t>(p.out) | reinterpret_cast<uintptr_t>(p.dout) |
                           reinterpret_cast<uintptr_t>(p.dgx) | reinterpret_cast<uintptr_t>(p.dq);
    const bool vec = (H & 3) == 0 && (ptrs & 15) == 0;
    const bool vec2 = !vec && (H & 1) == 0 && (ptrs & 7) == 0;          // H % 4 == 2 (MatchTensor's 70): 8-byte pieces, two per row
    auto load_cells = [&](int step, CellIn& ci) {
        const bool on_ = step >= 0 && step < len;
        const int st_ = on_ ? step : 0;
        const int t_ = dir == 0 ? st_ : (len > 0 ? len - 1 - st_ : 0);
        const int64_t row_ = mrow * T + t_;
        const float* a = p.act + (row_ * ND + dir) * (int64_t)H4;
        int tp = dir == 0 ? t_ - 1 : t_ + 1;                            // position of h_{t-1} (used when st_ > 0)
        tp = tp < 0 ? 0 : (tp >= T ? T - 1 : tp);
        const float* hpv = p.out + (mrow * T + tp) * ldo + dir * H;
        const float* dyp = p.dout + row_ * ldo + dir * H;
        const bool first = st_ == 0;
        if (vec) {
            const int u = ub < H ? ub : 0;
            auto ld4 = [&](const float* q, float (&dst)[4]) {
                const float4 v = *reinterpret_cast<const float4*>(q + u);
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
            };
#pragma unroll
            for (int g = 0; g < 4; ++g) ld4(a + g * H, ci.a[g]);
            ld4(hpv, ci.hp);
            ld4(dyp, ci.dy);
        } else if (vec2) {
            const int u0 = ub < H ? ub : 0, u1 = ub + 2 < H ? ub + 2 : u0;          // units past H: any valid address (masked below)
            auto ld22 = [&](const float* q, float (&dst)[4]) {
                const float2 v0 = *reinterpret_cast<const float2*>(q + u0), v1 = *reinterpret_cast<const float2*>(q + u1);
                dst[0] = v0.x; dst[1] = v0.y; dst[2] = v1.x; dst[3] = v1.y;
            };
#pragma unroll
            for (int g = 0; g < 4; ++g) ld22(a + g * H, ci.a[g]);
            ld22(hpv, ci.hp);
            ld22(dyp, ci.dy);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int u = ub + r < H ? ub + r : H - 1;
#pragma unroll
                for (int g = 0; g < 4; ++g) ci.a[g][r] = a[g * H + u];
                ci.hp[r] = hpv[u];
                ci.dy[r] = dyp[u];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) ci.hp[r] = first ? 0.f : ci.hp[r];
    };
    CellIn cin;
    load_cells(tmax - 1, cin);
    for (int step = tmax - 1; step >= 0; --step) {
        float* dgw = dgs + (step & 1) * SEQ * 4 * RS;
        const bool on = step < len;                                    // this sequence takes part in the step
        const int t = dir == 0 ? step : len - 1 - step;
        const int64_t row = mrow * T + (on ? t : 0);
        float gv[3][4], gq[4], dhd[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int u = ub + r;
            const bool cv = on && sv && u < H;
            const float r_ = cin.a[0][r], z_ = cin.a[1][r], n_ = cin.a[2][r], q_ = cin.a[3][r];
            const float dht = cin.dy[r] + dh[r];
            const float dan = dht * (1.f - z_) * (1.f - n_ * n_);
            gv[0][r] = cv ? dan * q_ * r_ * (1.f - r_) : 0.f;
            gv[1][r] = cv ? dht * (cin.hp[r] - n_) * z_ * (1.f - z_) : 0.f;
            gv[2][r] = cv ? dan : 0.f;
            gq[r] = cv ? dan * r_ : 0.f;
            dhd[r] = cv ? dht * z_ : 0.f;
            // B operand: k-step (g, c = u / 4), kq = r  ->  dgw[sq][r][g KG + c]   (zero for padded units / idle sequences)
            if (u < HP) {
                float* d = dgw + (sq * 4 + r) * RS + (u >> 2);
                d[0] = gv[0][r]; d[KG] = gv[1][r]; d[2 * KG] = gq[r];
            }
            if (cv && !vec && !vec2) {
                float* o = p.dgx + row * (int64_t)(ND * H3) + dir * H3;
                o[u] = gv[0][r]; o[H + u] = gv[1][r]; o[2 * H + u] = gv[2][r];
                p.dq[row * ldo + dir * H + u] = gq[r];
            }
        }
        if (vec && on && sv && ub < H) {
            float* o = p.dgx + row * (int64_t)(ND * H3) + dir * H3 + ub;
#pragma unroll
            for (int g = 0; g < 3; ++g) *reinterpret_cast<float4*>(o + g * H) = make_float4(gv[g][0], gv[g][1], gv[g][2], gv[g][3]);
            *reinterpret_cast<float4*>(p.dq + row * ldo + dir * H + ub) = make_float4(gq[0], gq[1], gq[2], gq[3]);
        }
        if (vec2 && on && sv && ub < H) {
            float* o = p.dgx + row * (int64_t)(ND * H3) + dir * H3 + ub;
            float* oq = p.dq + row * ldo + dir * H + ub;
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                *reinterpret_cast<float2*>(o + g * H) = make_float2(gv[g][0], gv[g][1]);
                if (ub + 2 < H) *reinterpret_cast<float2*>(o + g * H + 2) = make_float2(gv[g][2], gv[g][3]);
            }
            *reinterpret_cast<float2*>(oq) = make_float2(gq[0], gq[1]);
            if (ub + 2 < H) *reinterpret_cast<float2*>(oq + 2) = make_float2(gq[2], gq[3]);
        }
        load_cells(step - 1, cin);                                     // lands under this step's MFMAs
        lds_barrier();                                   // LDS only: the prefetched cell inputs and the gradient stores stay in flight under the MFMAs
        f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float* bp = dgw + (sq * 4 + pq) * RS;
#pragma unroll
        for (int k4 = 0; k4 < NKS / 4; ++k4) {
            const float4 b = *reinterpret_cast<const float4*>(bp + 4 * k4);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(afr[4 * k4 + 0], b.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(afr[4 * k4 + 1], b.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(afr[4 * k4 + 2], b.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(afr[4 * k4 + 3], b.w, acc1, 0, 0, 0);
        }
        // sequences that have not started yet (step >= len) keep the final-state gradient
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (on) dh[r] = dhd[r] + (acc0[r] + acc1[r]);
    }
    // zero the gradients of the padded steps: one wave per (sequence, step) row, coalesced
    __syncthreads();
    for (int s_ = 0; s_ < SEQ && m0 + s_ < p.M; ++s_)
        for (int t2 = lens_s[s_] + wave; t2 < T; t2 += NWV) {
            const int64_t row = (m0 + s_) * T + t2;
            float* o = p.dgx + row * (int64_t)(ND * H3) + dir * H3;
            for (int col = lane; col < H3; col += 64) o[col] = 0.f;
            float* oq = p.dq + row * ldo + dir * H;
            for (int col = lane; col < H; col += 64) oq[col] = 0.f;
        }
}

template <int HP>
static void gru_bwd_mfma_launch(const GruBwdArgs& a, hipStream_t st) {
    constexpr int NKS = (3 * (HP / 4) + 3) / 4 * 4;
    const size_t lds = (size_t)2 * 16 * 4 * (NKS + 4) * 4 + 16 * 4;
    hipLaunchKernelGGL(gru_train_bwd_mfma_kernel<HP>, dim3((unsigned)((a.M + 15) / 16), (unsigned)a.ND), dim3(64 * ((HP + 15) / 16)), lds, st, a);
}

// ---------------------------------------------------------------------------------------------------------------------
// The cell inside [B,T,.] sequence buffers (autograd._GRUSeq; any H): the step's gates are gx (row stride ldgx: the input projection of all steps)
// and gh ([B,3H] contiguous: the recurrent GEMM of this step, b_hh included; NULL: b_hh alone -- the first step, h_{t-1} = 0); act / h are written
// into the step's columns of the sequence buffers.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void gru_cell_seq_fwd_kernel(const float* __restrict__ gx, int64_t ldgx, const float* __restrict__ gh, const float* __restrict__ bhh,
                                        const float* __restrict__ hprev, int64_t ldhp, float* __restrict__ act, int64_t ldact, float* __restrict__ h,
                                        int64_t ldh, int64_t B, int H) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H) return;
    const int64_t b = i / H;
    const int j = (int)(i % H);
    const float* xr = gx + b * ldgx;
    float g[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) g[q] = gh ? gh[b * 3 * H + q * H + j] : (bhh ? bhh[q * H + j] : 0.f);
    const float r = 1.0f / (1.0f + expf(-(xr[j] + g[0]))), z = 1.0f / (1.0f + expf(-(xr[H + j] + g[1])));
    const float n = tanhf(xr[2 * H + j] + r * g[2]);
    float* ar = act + b * ldact;
    ar[j] = r; ar[H + j] = z; ar[2 * H + j] = n; ar[3 * H + j] = g[2];
    h[b * ldh + j] = (1.f - z) * n + z * (hprev ? hprev[b * ldhp + j] : 0.f);
}
// dh = dh_step (strided, the consumers of this step's h) + dh_rec (contiguous, dgh_{t+1} W_hh) + dh_dir (contiguous, z dh of step t+1); any may
// be NULL.  -> dgx (row stride lddgx), dgh (row stride lddgh: the A operand of the next recurrent GEMM and of the weight gradient), z dh [B,H]
__global__ void gru_cell_seq_bwd_kernel(const float* __restrict__ dh1, int64_t ld1, const float* __restrict__ dh2, const float* __restrict__ dh3,
                                        const float* __restrict__ act, int64_t ldact, const float* __restrict__ hprev, int64_t ldhp,
                                        float* __restrict__ dgx, int64_t lddgx, float* __restrict__ dgh, int64_t lddgh, float* __restrict__ dhdir,
                                        int64_t B, int H) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H) return;
    const int64_t b = i / H;
    const int j = (int)(i % H);
    const float* ar = act + b * ldact;
    const float r = ar[j], z = ar[H + j], n = ar[2 * H + j], q = ar[3 * H + j];
    const float dh = (dh1 ? dh1[b * ld1 + j] : 0.f) + (dh2 ? dh2[i] : 0.f) + (dh3 ? dh3[i] : 0.f);
    const float dan = dh * (1.f - z) * (1.f - n * n);
    const float da_r = dan * q * r * (1.f - r);
    const float da_z = dh * ((hprev ? hprev[b * ldhp + j] : 0.f) - n) * z * (1.f - z);
    float* ox = dgx + b * lddgx;
    ox[j] = da_r; ox[H + j] = da_z; ox[2 * H + j] = dan;
    float* oh = dgh + b * lddgh;
    oh[j] = da_r; oh[H + j] = da_z; oh[2 * H + j] = dan * r;
    dhdir[i] = dh * z;
}

}  // namespace nir

extern "C" int nir_gru_train_mfma_supported(int H) {
    const int hp = (H + 3) / 4 * 4;
    return (H >= 16 && H <= 128 && (hp == 32 || hp == 64 || hp == 72 || hp == 96 || hp == 128)) ? 1 : 0;
}

// NIR_GRU_FORM_AUTO: the dispatch of nir_lstm_train_bwd -- the matrix-core form for the hidden sizes it takes; odd H has no 8-byte cell IO and
// goes there from 1024 sequences on only (measured for the LSTM's BPTT, not re-measured for the GRU)
static int gru_pick_form(int form, int64_t M, int H) {
    if (form != NIR_GRU_FORM_AUTO) return form;
    return (nir_gru_train_mfma_supported(H) && (H % 2 == 0 || M >= 1024)) ? NIR_GRU_FORM_MFMA : NIR_GRU_FORM_VALU;
}

extern "C" int nir_gru_train_fwd(const float* gates_in, const int64_t* lengths, const float* w_hh, const float* b_hh, float* out, float* act, float* hn,
                                 int64_t M, int T, int H, int ndir, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(gates_in && w_hh && b_hh && out && act, "gru_train_fwd: null pointer");
    NIR_REQUIRE(M >= 0 && T > 0 && (ndir == 1 || ndir == 2) && H >= 1 && H <= 128, "gru_train_fwd: bad dims (H <= 128)");
    if (M == 0) return 0;
    GruTrainArgs a{gates_in, lengths, w_hh, b_hh, out, act, hn, M, T, H, ndir};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((M + GSQ - 1) / GSQ), (unsigned)ndir);
    const int threads = (3 * H + 63) / 64 * 64;
    const size_t lds = (size_t)GSQ * 4 * H * 4;
    ProfScope ps(prof_shape_name("gru_train_fwd_kernel", M, T, H), st);
    if (H <= 32) hipLaunchKernelGGL(gru_train_fwd_kernel<32>, grid, dim3(threads), lds, st, a);
    else if (H <= 64) hipLaunchKernelGGL(gru_train_fwd_kernel<64>, grid, dim3(threads), lds, st, a);
    else if (H <= 96) hipLaunchKernelGGL(gru_train_fwd_kernel<96>, grid, dim3(threads), lds, st, a);
    else hipLaunchKernelGGL(gru_train_fwd_kernel<128>, grid, dim3(threads), lds, st, a);
    NIR_CHECK_LAUNCH("gru_train_fwd_kernel");
    return 0;
}

extern "C" int nir_gru_train_bwd(const float* dout, const float* dhn, const float* act, const float* out, const int64_t* lengths, const float* w_hh,
                                 float* dgx, float* dq, int64_t M, int T, int H, int ndir, int form, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(dout && act && out && w_hh && dgx && dq, "gru_train_bwd: null pointer");
    NIR_REQUIRE(M >= 0 && T > 0 && (ndir == 1 || ndir == 2) && H >= 1 && H <= 128, "gru_train_bwd: bad dims (H <= 128)");
    NIR_REQUIRE(form == NIR_GRU_FORM_AUTO || form == NIR_GRU_FORM_VALU || form == NIR_GRU_FORM_MFMA, "gru_train_bwd: bad form %d", form);
    const int hp = (H + 3) / 4 * 4;
    NIR_REQUIRE(form != NIR_GRU_FORM_MFMA || nir_gru_train_mfma_supported(H), "gru_train_bwd: the matrix-core form takes H rounded up to 4 in {32, 64, 72, 96, 128} (got H = %d)", H);
    if (M == 0) return 0;
    form = gru_pick_form(form, M, H);
    GruBwdArgs a{dout, dhn, act, out, lengths, w_hh, dgx, dq, M, T, H, ndir};
    hipStream_t st = (hipStream_t)stream;
    if (form == NIR_GRU_FORM_MFMA) {
        ProfScope ps(prof_shape_name("gru_train_bwd_mfma_kernel", M, T, H), st);
        if (hp == 32) gru_bwd_mfma_launch<32>(a, st);
        else if (hp == 64) gru_bwd_mfma_launch<64>(a, st);
        else if (hp == 72) gru_bwd_mfma_launch<72>(a, st);
        else if (hp == 96) gru_bwd_mfma_launch<96>(a, st);
        else gru_bwd_mfma_launch<128>(a, st);
        NIR_CHECK_LAUNCH("gru_train_bwd_mfma_kernel");
        return 0;
    }
    const int threads = (3 * H + 63) / 64 * 64;
    const size_t lds = (size_t)GSQ * (3 * H + H + 3 * H) * 4;
    ProfScope ps(prof_shape_name("gru_train_bwd_kernel", M, T, H), st);
    hipLaunchKernelGGL(gru_train_bwd_kernel, dim3((unsigned)((M + GSQ - 1) / GSQ), (unsigned)ndir), dim3(threads), lds, st, a);
    NIR_CHECK_LAUNCH("gru_train_bwd_kernel");
    return 0;
}

extern "C" int nir_gru_cell_seq_fwd(const float* gx, int64_t ldgx, const float* gh, const float* b_hh, const float* h_prev, int64_t ldhp, float* act,
                                    int64_t ldact, float* h, int64_t ldh, int64_t B, int H, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(gx && act && h && (gh || b_hh), "gru_cell_seq_fwd: null pointer");
    NIR_REQUIRE(B >= 0 && H > 0 && ldgx >= 3 * (int64_t)H && ldact >= 4 * (int64_t)H && ldh >= H && (!h_prev || ldhp >= H), "gru_cell_seq_fwd: bad dims");
    if (B == 0) return 0;
    hipLaunchKernelGGL(gru_cell_seq_fwd_kernel, g1(B * H), dim3(256), 0, (hipStream_t)stream, gx, ldgx, gh, b_hh, h_prev, ldhp, act, ldact, h, ldh, B, H);
    NIR_CHECK_LAUNCH("gru_cell_seq_fwd_kernel");
    return 0;
}

extern "C" int nir_gru_cell_seq_bwd(const float* dh_step, int64_t ld_dh, const float* dh_rec, const float* dh_dir, const float* act, int64_t ldact,
                                    const float* h_prev, int64_t ldhp, float* dgx, int64_t lddgx, float* dgh, int64_t lddgh, float* dh_dir_out, int64_t B,
                                    int H, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(act && dgx && dgh && dh_dir_out, "gru_cell_seq_bwd: null pointer");
    NIR_REQUIRE(B >= 0 && H > 0 && ldact >= 4 * (int64_t)H && lddgx >= 3 * (int64_t)H && lddgh >= 3 * (int64_t)H && (!dh_step || ld_dh >= H) &&
                    (!h_prev || ldhp >= H), "gru_cell_seq_bwd: bad dims");
    if (B == 0) return 0;
    hipLaunchKernelGGL(gru_cell_seq_bwd_kernel, g1(B * H), dim3(256), 0, (hipStream_t)stream, dh_step, ld_dh, dh_rec, dh_dir, act, ldact, h_prev, ldhp, dgx,
                       lddgx, dgh, lddgh, dh_dir_out, B, H);
    NIR_CHECK_LAUNCH("gru_cell_seq_bwd_kernel");
    return 0;
}
