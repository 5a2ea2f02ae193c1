// DSSM and CDSSM rankers (neuroir/rankers/dssm.py:33-63, neuroir/rankers/cdssm.py:42-77) and the operators of their training step.
//
// Both models ignore the lengths and max-pool over the PADDED positions.  Every position (DSSM) or 5-token window (CDSSM) made only of
// PAD ids yields the same vector, so a row is evaluated up to its last non-PAD id only (read from the ids, never from *_len) and the
// all-PAD vector -- the PAD row of the table for DSSM, the tower applied to a window of PAD ids for CDSSM -- is folded into the max of
// every row that has such a tail.  Exact: max ignores order and repetition.
//
// Arithmetic is fp32 FMA throughout (exact-fp32 class; tanhf, not the exp2 approximation): no fp16 / bf16 operand terms.
//
//   dssm_tower_kernel   one row per workgroup (query and document rows in one launch; the block index selects the tower):
//                       gather + max over the effective positions (+ the PAD row), Linear -> tanh -> Linear -> tanh, rep [rows, NO]
//   cdssm_tile_kernel   one (row, tile of 32 window positions) per workgroup: 5-tap conv as a gathered GEMM from an LDS tile of table rows
//                       (packed fp32 FMA, two windows per instruction), bias + tanh kept in LDS, Linear(NH -> NO) + tanh, column max over the tile -> partial [rows, tiles, NO];
//                       tiles past the effective length exit at once; two extra workgroups evaluate the all-PAD window of each tower
//   rank_finish_kernel  one wave per (query, candidate): max over the tiles (+ the all-PAD vector), ATen cosine -> scores [B, N]
#include "split2.hpp"
#include <algorithm>

namespace nir {

constexpr int CD_TP = 32;          // window positions per cdssm_tile_kernel workgroup (LDS 48 KB at E = 300: 3 workgroups per CU)
constexpr int CD_TAPS = 5;         // Conv1d(k=3) over the 3-row interleave = a 5-row window (cdssm.py:33-41)
constexpr int CD_THREADS = 320;    // one GEMM-1 column per thread at NH <= 320
constexpr int CD_HALF = CD_TP / 2;  // GEMM 1 pairs window p with window p + CD_HALF
constexpr int CD_NQ = CD_HALF + CD_TAPS - 1;
constexpr int DS_INFLIGHT = 8;     // table rows a dssm_tower_kernel wave has in flight

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s, 64));
    return v;
}

// index of the last id != pad in ids[0, L) (-1 if none), computed by one wave
__device__ __forceinline__ int wave_last_nonpad(const int64_t* ids, int L, int64_t pad, int lane) {
    int last = -1;
    for (int i = lane; i < L; i += 64)
        if (ids[i] != pad) last = i;
    return wave_max_i(last);
}

struct DssmTower {
    const float *w1t, *b1, *w2t, *b2;   // w1t [E][NH], w2t [NH][NO] (transposed Linear weights)
};

// One row per workgroup: rows [0, nq) of the query tower in blocks [0, nq), rows [0, nd) of the document tower after them.
// Gather: wave w takes the 64-position chunks w, w + 4, ..; a lane loads one id of the chunk, the wave then reads DS_INFLIGHT table rows per
// round (row addresses by shuffle, no dependent id load per row); the four per-wave maxima meet in LDS.
__global__ __launch_bounds__(256) void dssm_tower_kernel(const int64_t* q_ids, int QL, int64_t nq, const int64_t* d_ids, int DL, int64_t nd,
                                                         const float* table, int E, int64_t pad, DssmTower tq, DssmTower td, int NH, int NO,
                                                         float* rep_q, float* rep_d) {
    extern __shared__ float sm[];
    float* red = sm;                // [4][E] per-wave maxima
    float* xs = sm + 4 * E;         // [E]
    float* hs = xs + E;             // [NH]
    __shared__ int s_last;
    const bool isq = (int64_t)blockIdx.x < nq;
    const int64_t r = isq ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - nq;
    const int L = isq ? QL : DL;
    const int64_t* rid = (isq ? q_ids : d_ids) + r * L;
    const DssmTower w = isq ? tq : td;
    float* rep = isq ? rep_q : rep_d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {
        const int last = wave_last_nonpad(rid, L, pad, lane);
        if (lane == 0) s_last = last;
    }
    __syncthreads();
    const int last = s_last;
    // gather + max (dssm.py:46-55) over positions [0, last]; lane owns columns lane + 64 j
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
    for (int base = wave * 64; base <= last; base += 256) {
        const int cnt = min(64, last + 1 - base);
        const int64_t myid = lane < cnt ? rid[base + lane] : pad;
        for (int i = 0; i < cnt; i += DS_INFLIGHT) {
            float v[DS_INFLIGHT][8];
#pragma unroll
            for (int k = 0; k < DS_INFLIGHT; ++k) {
                const bool ok = i + k < cnt;
                const float* rp = table + __shfl(myid, ok ? i + k : 0, 64) * (int64_t)E;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = lane + 64 * j;
                    v[k][j] = (ok && c < E) ? rp[c] : -INFINITY;
                }
            }
#pragma unroll
            for (int k = 0; k < DS_INFLIGHT; ++k)
#pragma unroll
                for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], v[k][j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = lane + 64 * j;
        if (c < E) red[wave * E + c] = m[j];
    }
    __syncthreads();
    const bool padded = last < L - 1;            // the max also runs over the PAD tail: its value is the PAD row
    for (int c = threadIdx.x; c < E; c += 256) {
        float x = fmaxf(fmaxf(red[c], red[E + c]), fmaxf(red[2 * E + c], red[3 * E + c]));
        if (padded) x = fmaxf(x, table[pad * (int64_t)E + c]);
        xs[c] = x;
    }
    __syncthreads();
    // Linear(E -> NH) + tanh (dssm.py:20-25), then Linear(NH -> NO) + tanh; weight loads batched 8 deep
    for (int o = threadIdx.x; o < NH; o += 256) {
        float acc = w.b1[o];
        int k = 0;
        for (; k + 8 <= E; k += 8) {
            float wk[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) wk[u] = w.w1t[(int64_t)(k + u) * NH + o];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fmaf(wk[u], xs[k + u], acc);
        }
        for (; k < E; ++k) acc = fmaf(w.w1t[(int64_t)k * NH + o], xs[k], acc);
        hs[o] = tanhf(acc);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < NO; o += 256) {
        float acc = w.b2[o];
        int k = 0;
        for (; k + 8 <= NH; k += 8) {
            float wk[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) wk[u] = w.w2t[(int64_t)(k + u) * NO + o];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fmaf(wk[u], hs[k + u], acc);
        }
        for (; k < NH; ++k) acc = fmaf(w.w2t[(int64_t)k * NO + o], hs[k], acc);
        rep[r * NO + o] = tanhf(acc);
    }
}

struct CdssmTower {
    const float *w5t, *b, *semt, *semb;  // w5t [5E][NH] (k = tap * E + e, the folded 5-tap conv), semt [NH][NO]
};

// Block layout: [0, B*Tq) query tiles, [B*Tq, B*Tq + M*Td) document tiles, then the all-PAD window of the query and of the document tower.
// partial_q [B][Tq][NO], partial_d [M][Td][NO], padvec [2][NO].
__global__ __launch_bounds__(CD_THREADS) void cdssm_tile_kernel(const int64_t* q_ids, int QL, int64_t B, int Tq, const int64_t* d_ids, int DL,
                                                                int64_t M, int Td, const float* table, int E, int64_t pad, CdssmTower tq,
                                                                CdssmTower td, int NH, int NO, float* part_q, float* part_d, float* padvec) {
    extern __shared__ float4 sm4[];
    float* sm = reinterpret_cast<float*>(sm4);
    __shared__ int s_last;
    const int64_t nqb = B * Tq, ndb = M * Td;
    const int64_t bid = blockIdx.x;
    bool isq;
    int64_t row;
    int tile, L, P;
    const int64_t* rid;
    float* out;
    if (bid < nqb) {
        isq = true, row = bid / Tq, tile = (int)(bid % Tq), L = QL, rid = q_ids + row * QL;
        out = part_q + (row * Tq + tile) * NO;
    } else if (bid < nqb + ndb) {
        isq = false, row = (bid - nqb) / Td, tile = (int)((bid - nqb) % Td), L = DL, rid = d_ids + row * DL;
        out = part_d + (row * Td + tile) * NO;
    } else {                                   // the all-PAD window of a tower
        isq = bid == nqb + ndb, row = 0, tile = 0, L = CD_TAPS, rid = nullptr;
        out = padvec + (isq ? 0 : NO);
    }
    P = L - CD_TAPS + 1;
    const CdssmTower w = isq ? tq : td;
    const int tid = threadIdx.x;
    int peff = 1;
    if (rid) {
        if (tid < 64) {
            const int last = wave_last_nonpad(rid, L, pad, tid);
            if (tid == 0) s_last = last;
        }
        __syncthreads();
        peff = min(P, s_last + 1);          // windows j > last are all PAD
    }
    const int p0 = tile * CD_TP;
    if (p0 >= peff) return;                  // (uniform) the rank_finish_kernel never reads this tile
    // xt[e][2 q + h] = table[id(p0 + q + h CD_HALF)][e], q < CD_NQ: the rows of the two window halves side by side, so that one 64-bit register
    // pair holds the operands of windows p and p + CD_HALF for one packed FMA (rows CD_HALF .. CD_NQ-1 are stored twice)
    const int ld = 2 * CD_NQ;                // 40 floats: 16-byte aligned rows
    float* xt = sm;
    for (int sl = tid / 64; sl < ld; sl += CD_THREADS / 64) {
        const int pos = p0 + (sl >> 1) + (sl & 1) * CD_HALF;
        const bool in = pos < L;
        const int64_t id = rid ? (in ? rid[pos] : pad) : pad;
        const float* src = table + id * (int64_t)E;
        for (int e = tid & 63; e < E; e += 64) xt[e * ld + sl] = in ? src[e] : 0.f;
    }
    __syncthreads();
    // GEMM 1: h[p][o] = tanh(b[o] + sum_{m<5, e<E} w5[o][m][e] x[p + m][e])   (cdssm.py:60-62 with the interleave folded into 5 taps);
    // thread o owns column o for all CD_TP windows of the tile, as CD_HALF packed pairs (v_pk_fma_f32: windows p and p + CD_HALF)
    float* ht = sm;                          // [NH][CD_TP], overlays xt after the barrier below
    const int o = tid;
    f32x2 acc[CD_HALF];
    if (o < NH) {
        const float bo = w.b[o];
#pragma unroll
        for (int p = 0; p < CD_HALF; ++p) acc[p] = f32x2{bo, bo};
        float wn[CD_TAPS];                   // the next e's weights are in flight while this e's products run
#pragma unroll
        for (int m = 0; m < CD_TAPS; ++m) wn[m] = w.w5t[(int64_t)m * E * NH + o];
        for (int e = 0; e < E; ++e) {
            float wc[CD_TAPS];
#pragma unroll
            for (int m = 0; m < CD_TAPS; ++m) wc[m] = wn[m];
            if (e + 1 < E) {
#pragma unroll
                for (int m = 0; m < CD_TAPS; ++m) wn[m] = w.w5t[((int64_t)m * E + e + 1) * NH + o];
            }
            f32x2 x[CD_NQ];
            const float4* xr = reinterpret_cast<const float4*>(xt + e * ld);
#pragma unroll
            for (int q = 0; q < CD_NQ / 2; ++q) {
                const float4 v = xr[q];
                x[2 * q] = f32x2{v.x, v.y}, x[2 * q + 1] = f32x2{v.z, v.w};
            }
#pragma unroll
            for (int m = 0; m < CD_TAPS; ++m) {
                const f32x2 wm = f32x2{wc[m], wc[m]};
#pragma unroll
                for (int p = 0; p < CD_HALF; ++p) acc[p] = __builtin_elementwise_fma(wm, x[p + m], acc[p]);
            }
        }
#pragma unroll
        for (int p = 0; p < CD_HALF; ++p) acc[p] = f32x2{tanhf(acc[p].x), tanhf(acc[p].y)};
    }
    __syncthreads();                         // every thread is done with xt
    if (o < NH) {
        float* hw = ht + (int64_t)o * CD_TP;
#pragma unroll
        for (int q = 0; q < CD_HALF / 4; ++q) {
            reinterpret_cast<float4*>(hw)[q] = make_float4(acc[4 * q].x, acc[4 * q + 1].x, acc[4 * q + 2].x, acc[4 * q + 3].x);
            reinterpret_cast<float4*>(hw + CD_HALF)[q] = make_float4(acc[4 * q].y, acc[4 * q + 1].y, acc[4 * q + 2].y, acc[4 * q + 3].y);
        }
    }
    __syncthreads();
    // GEMM 2: y[p][c] = tanh(semb[c] + sum_o sem[c][o] h[p][o]) (cdssm.py:62), then the column max over this tile's valid windows (cdssm.py:63)
    float* red = sm + (int64_t)NH * CD_TP;   // [2][NO]
    const int nvalid = min(CD_TP, peff - p0);
    for (int it = tid; it < 2 * NO; it += CD_THREADS) {
        const int c = it % NO, half = it / NO;
        float acc[CD_TP / 2];
        const float bc = w.semb[c];
#pragma unroll
        for (int p = 0; p < CD_TP / 2; ++p) acc[p] = bc;
        for (int k = 0; k < NH; ++k) {
            const float wk = w.semt[(int64_t)k * NO + c];
            const float4* hr = reinterpret_cast<const float4*>(ht + (int64_t)k * CD_TP + half * (CD_TP / 2));
#pragma unroll
            for (int q = 0; q < CD_TP / 8; ++q) {
                const float4 v = hr[q];
                acc[4 * q] = fmaf(wk, v.x, acc[4 * q]);
                acc[4 * q + 1] = fmaf(wk, v.y, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(wk, v.z, acc[4 * q + 2]);
                acc[4 * q + 3] = fmaf(wk, v.w, acc[4 * q + 3]);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int p = 0; p < CD_TP / 2; ++p)
            if (half * (CD_TP / 2) + p < nvalid) mx = fmaxf(mx, tanhf(acc[p]));
        red[half * NO + c] = mx;
    }
    __syncthreads();
    for (int c = tid; c < NO; c += CD_THREADS) out[c] = fmaxf(red[c], red[NO + c]);
}

// One wave per (b, n): rq = max over the Tq partial rows of query b (+ padvec_q), rd likewise for candidate (b, n); ATen cosine
// x/max(|x|,1e-8) . y/max(|y|,1e-8).  ids == NULL: every tile counts and nothing is folded (T = 1 gives the plain broadcast cosine).
// With ids, the valid tiles of a row follow from its last non-PAD id (window count P = L - taps + 1; taps = 5 for CDSSM).
__global__ __launch_bounds__(256) void rank_finish_kernel(const float* part_q, int Tq, const float* part_d, int Td, const int64_t* q_ids, int QL,
                                                          const int64_t* d_ids, int DL, int64_t pad, int taps, const float* padvec, int64_t B,
                                                          int N, int NO, float* scores, float* rep_q, float* rep_d) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= B * N) return;
    const int64_t b = pair / N;
    int tq = Tq, td = Td;
    bool fq = false, fd = false;
    if (q_ids) {
        const int Pq = QL - taps + 1, Pd = DL - taps + 1;
        const int eq = min(Pq, wave_last_nonpad(q_ids + b * QL, QL, pad, lane) + 1);
        const int ed = min(Pd, wave_last_nonpad(d_ids + pair * DL, DL, pad, lane) + 1);
        tq = (eq + CD_TP - 1) / CD_TP, td = (ed + CD_TP - 1) / CD_TP;
        fq = eq < Pq, fd = ed < Pd;
    }
    float rq[4], rd[4];
    float nq = 0.f, nd = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane + 64 * j;
        float a = -INFINITY, d = -INFINITY;
        if (c < NO) {
            for (int t = 0; t < tq; ++t) a = fmaxf(a, part_q[(b * Tq + t) * NO + c]);
            for (int t = 0; t < td; ++t) d = fmaxf(d, part_d[(pair * Td + t) * NO + c]);
            if (fq) a = fmaxf(a, padvec[c]);
            if (fd) d = fmaxf(d, padvec[NO + c]);
            if (rep_q && pair % N == 0) rep_q[b * NO + c] = a;
            if (rep_d) rep_d[pair * NO + c] = d;
        } else {
            a = d = 0.f;
        }
        rq[j] = a, rd[j] = d;
        nq = fmaf(a, a, nq), nd = fmaf(d, d, nd);
    }
    nq = fmaxf(sqrtf(wave_sum(nq)), 1e-8f);
    nd = fmaxf(sqrtf(wave_sum(nd)), 1e-8f);
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) dot = fmaf(rq[j] / nq, rd[j] / nd, dot);
    dot = wave_sum(dot);
    if (lane == 0) scores[pair] = dot;
}

// ---- training operators ---------------------------------------------------------------------------------------------------------------

// y[r][d] = max_t x[r][t][d], idx[r][d] = the first arg-max (dssm.py:49,55; cdssm.py:63,71)
__global__ __launch_bounds__(256) void maxpool_arg_kernel(const float* x, int64_t R, int T, int D, float* y, int* idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R * D) return;
    const int64_t r = i / D;
    const int d = (int)(i % D);
    const float* xr = x + r * T * (int64_t)D + d;
    float best = xr[0];
    int arg = 0;
    for (int t = 1; t < T; ++t) {
        const float v = xr[(int64_t)t * D];
        if (v > best) best = v, arg = t;
    }
    y[i] = best;
    idx[i] = arg;
}

// dx[r][t][d] = dy[r][d] at t = idx[r][d], else 0 (every element written: no separate zero fill)
__global__ __launch_bounds__(256) void maxpool_arg_bwd_kernel(const float* dy, const int* idx, int64_t R, int T, int D, float* dx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R * D) return;
    const int64_t r = i / D;
    const int d = (int)(i % D);
    const int a = idx[i];
    const float g = dy[i];
    float* xr = dx + r * T * (int64_t)D + d;
    for (int t = 0; t < T; ++t) xr[(int64_t)t * D] = t == a ? g : 0.f;
}

// One wave per query b: s_bn = x.y / (max(|x|,eps) max(|y|,eps)) with x = q[b], y = d[b][n];
//   ds/dx = y/(nx ny) - s x/nx^2 when |x| > eps, y/(eps ny) otherwise (the clamp is constant there); dq[b] sums over the N candidates.
__global__ __launch_bounds__(256) void cosine_bcast_bwd_kernel(const float* q, const float* d, const float* g, int64_t B, int N, int D,
                                                               float* dq, float* dd) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float eps = 1e-8f;
    float x[8], aq[8];
    float xx = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = lane + 64 * j;
        x[j] = c < D ? q[b * D + c] : 0.f;
        aq[j] = 0.f;
        xx = fmaf(x[j], x[j], xx);
    }
    const float xn = sqrtf(wave_sum(xx));
    const float nx = fmaxf(xn, eps);
    for (int n = 0; n < N; ++n) {
        const float* yr = d + (b * N + n) * (int64_t)D;
        float y[8];
        float yy = 0.f, xy = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = lane + 64 * j;
            y[j] = c < D ? yr[c] : 0.f;
            yy = fmaf(y[j], y[j], yy);
            xy = fmaf(x[j], y[j], xy);
        }
        const float yn = sqrtf(wave_sum(yy));
        const float ny = fmaxf(yn, eps);
        xy = wave_sum(xy);
        const float s = xy / (nx * ny);
        const float gs = g[b * N + n];
        const float cx = xn > eps ? s / (nx * nx) : 0.f;
        const float cy = yn > eps ? s / (ny * ny) : 0.f;
        float* dr = dd + (b * N + n) * (int64_t)D;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = lane + 64 * j;
            if (c < D) {
                aq[j] = fmaf(gs, y[j] / (nx * ny) - cx * x[j], aq[j]);
                dr[c] = gs * (x[j] / (nx * ny) - cy * y[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = lane + 64 * j;
        if (c < D) dq[b * D + c] = aq[j];
    }
}

// d/ds of -(log_softmax(s) . y).sum(1).mean()  (models/ranker.py:79-89):  ds = g (softmax(s) sum_j y_j - y) / R;  one wave per row
__global__ __launch_bounds__(256) void softmax_nll_bwd_kernel(const float* s, const float* y, const float* g, int64_t R, int n, float* ds) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float* x = s + r * n;
    const float* t = y + r * n;
    float mx = -INFINITY;
    for (int i = lane; i < n; i += 64) mx = fmaxf(mx, x[i]);
    mx = wave_max(mx);
    float se = 0.f, sy = 0.f;
    for (int i = lane; i < n; i += 64) se += expf(x[i] - mx), sy += t[i];
    se = wave_sum(se), sy = wave_sum(sy);
    const float k = g[0] / (float)R;
    for (int i = lane; i < n; i += 64) ds[r * n + i] = k * (expf(x[i] - mx) / se * sy - t[i]);
}

static size_t cdssm_tiles(int L) { return (size_t)((L - CD_TAPS + 1 + CD_TP - 1) / CD_TP); }

}  // namespace nir

extern "C" size_t nir_dssm_workspace_bytes(int B, int N, int NO) {
    return nir::align_up((size_t)B * NO * 4, 256) + nir::align_up((size_t)B * N * NO * 4, 256);
}

extern "C" int nir_dssm_score(const int64_t* q_ids, const int64_t* d_ids, int B, int N, int QL, int DL, const float* table, int64_t V, int E,
                              int64_t pad, const nir_dssm_weights* w, void* workspace, size_t workspace_bytes, float* scores, float* rep_q,
                              float* rep_d, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(q_ids && d_ids && table && w && scores, "dssm: null pointer");
    NIR_REQUIRE(B >= 0 && N > 0 && QL > 0 && DL > 0 && V > 0 && pad >= 0 && pad < V, "dssm: bad dims B=%d N=%d QL=%d DL=%d", B, N, QL, DL);
    NIR_REQUIRE(E > 0 && E <= 512 && w->NH > 0 && w->NO > 0 && w->NO <= 256, "dssm: emsize %d / nhid %d / nout %d unsupported (emsize <= 512, nout <= 256)",
                E, w->NH, w->NO);
    NIR_REQUIRE(w->q_w1t && w->q_b1 && w->q_w2t && w->q_b2 && w->d_w1t && w->d_b1 && w->d_w2t && w->d_b2, "dssm: null weight");
    if (B == 0) return 0;
    const int NH = w->NH, NO = w->NO;
    const int64_t M = (int64_t)B * N;
    Workspace ws(workspace, workspace_bytes);
    float* wq = ws.take<float>((size_t)B * NO);
    float* wd = ws.take<float>((size_t)M * NO);
    NIR_REQUIRE(ws.ok(), "dssm: workspace too small (%zu < %zu bytes)", workspace_bytes, ws.off);
    float* rq = rep_q ? rep_q : wq;
    float* rd = rep_d ? rep_d : wd;
    const size_t lds = (size_t)(5 * E + NH) * 4;
    NIR_REQUIRE(lds <= 64 * 1024, "dssm: emsize %d + nhid %d need %zu bytes of LDS", E, NH, lds);
    DssmTower tq{w->q_w1t, w->q_b1, w->q_w2t, w->q_b2}, td{w->d_w1t, w->d_b1, w->d_w2t, w->d_b2};
    {
        ProfScope ps("dssm_tower_kernel", (hipStream_t)stream);
        hipLaunchKernelGGL(dssm_tower_kernel, dim3((unsigned)(B + M)), dim3(256), lds, (hipStream_t)stream, q_ids, QL, (int64_t)B, d_ids, DL, M,
                           table, E, pad, tq, td, NH, NO, rq, rd);
        NIR_CHECK_LAUNCH("nir_dssm_score (tower)");
    }
    {
        ProfScope ps("rank_finish_kernel", (hipStream_t)stream);
        hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rq, 1, rd, 1, nullptr, QL,
                           nullptr, DL, pad, 1, nullptr, (int64_t)B, N, NO, scores, nullptr, nullptr);
        NIR_CHECK_LAUNCH("nir_dssm_score (finish)");
    }
    return 0;
}

extern "C" size_t nir_cdssm_workspace_bytes(int B, int N, int QL, int DL, int NO) {
    using namespace nir;
    if (QL < CD_TAPS || DL < CD_TAPS) return 0;
    return align_up((size_t)B * cdssm_tiles(QL) * NO * 4, 256) + align_up((size_t)B * N * cdssm_tiles(DL) * NO * 4, 256) +
           align_up((size_t)2 * NO * 4, 256);
}

extern "C" int nir_cdssm_score(const int64_t* q_ids, const int64_t* d_ids, int B, int N, int QL, int DL, const float* table, int64_t V, int E,
                               int64_t pad, const nir_cdssm_weights* w, void* workspace, size_t workspace_bytes, float* scores, float* rep_q,
                               float* rep_d, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(q_ids && d_ids && table && w && scores, "cdssm: null pointer");
    NIR_REQUIRE(QL >= CD_TAPS && DL >= CD_TAPS, "cdssm: query / document width %d / %d below the 5-token window of the 3-row interleave", QL, DL);
    NIR_REQUIRE(B >= 0 && N > 0 && V > 0 && pad >= 0 && pad < V, "cdssm: bad dims B=%d N=%d", B, N);
    NIR_REQUIRE(E > 0 && w->NH > 0 && w->NH <= CD_THREADS && w->NO > 0 && w->NO <= 256,
                "cdssm: nhid %d / nout %d unsupported (nhid <= %d, nout <= 256)", w->NH, w->NO, CD_THREADS);
    NIR_REQUIRE(w->q_w5t && w->q_b && w->q_semt && w->q_semb && w->d_w5t && w->d_b && w->d_semt && w->d_semb, "cdssm: null weight");
    if (B == 0) return 0;
    const int NH = w->NH, NO = w->NO;
    const int64_t M = (int64_t)B * N;
    const int Tq = (int)cdssm_tiles(QL), Td = (int)cdssm_tiles(DL);
    Workspace ws(workspace, workspace_bytes);
    float* pq = ws.take<float>((size_t)B * Tq * NO);
    float* pd = ws.take<float>((size_t)M * Td * NO);
    float* pv = ws.take<float>((size_t)2 * NO);
    NIR_REQUIRE(ws.ok(), "cdssm: workspace too small (%zu < %zu bytes)", workspace_bytes, ws.off);
    const size_t lds = (size_t)std::max((size_t)E * 2 * CD_NQ, (size_t)NH * CD_TP + 2 * NO) * 4;
    NIR_REQUIRE(lds <= 160 * 1024 - 1024, "cdssm: emsize %d / nhid %d need %zu bytes of LDS (> 159 KiB)", E, NH, lds);
    if (lds > 64 * 1024) {     // once per process: the largest size this entry accepts
        static const hipError_t e = hipFuncSetAttribute((const void*)cdssm_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
        if (e != hipSuccess) {
            set_error("cdssm: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e));
            return (int)e;
        }
    }
    CdssmTower tq{w->q_w5t, w->q_b, w->q_semt, w->q_semb}, td{w->d_w5t, w->d_b, w->d_semt, w->d_semb};
    {
        ProfScope ps("cdssm_tile_kernel", (hipStream_t)stream);
        hipLaunchKernelGGL(cdssm_tile_kernel, dim3((unsigned)(B * Tq + M * Td + 2)), dim3(CD_THREADS), lds, (hipStream_t)stream, q_ids, QL, (int64_t)B,
                           Tq, d_ids, DL, M, Td, table, E, pad, tq, td, NH, NO, pq, pd, pv);
        NIR_CHECK_LAUNCH("nir_cdssm_score (tiles)");
    }
    {
        ProfScope ps("rank_finish_kernel", (hipStream_t)stream);
        hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, pq, Tq, pd, Td, q_ids, QL, d_ids,
                           DL, pad, CD_TAPS, pv, (int64_t)B, N, NO, scores, rep_q, rep_d);
        NIR_CHECK_LAUNCH("nir_cdssm_score (finish)");
    }
    return 0;
}

extern "C" int nir_maxpool_arg_f32(const float* x, int64_t R, int T, int D, float* y, int* idx, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(x && y && idx && R >= 0 && T > 0 && D > 0, "maxpool_arg: bad args");
    if (R == 0) return 0;
    hipLaunchKernelGGL(maxpool_arg_kernel, dim3((unsigned)((R * D + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, R, T, D, y, idx);
    NIR_CHECK_LAUNCH("nir_maxpool_arg_f32");
    return 0;
}

extern "C" int nir_maxpool_arg_bwd_f32(const float* dy, const int* idx, int64_t R, int T, int D, float* dx, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(dy && idx && dx && R >= 0 && T > 0 && D > 0, "maxpool_arg_bwd: bad args");
    if (R == 0) return 0;
    hipLaunchKernelGGL(maxpool_arg_bwd_kernel, dim3((unsigned)((R * D + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, idx, R, T, D, dx);
    NIR_CHECK_LAUNCH("nir_maxpool_arg_bwd_f32");
    return 0;
}

extern "C" int nir_cosine_bcast_f32(const float* q, const float* d, int64_t B, int N, int D, float* s, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(q && d && s && B >= 0 && N > 0 && D > 0 && D <= 256, "cosine_bcast: bad args (D <= 256)");
    if (B == 0) return 0;
    hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)((B * N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, q, 1, d, 1, nullptr, 0, nullptr, 0,
                       (int64_t)0, 1, nullptr, B, N, D, s, nullptr, nullptr);
    NIR_CHECK_LAUNCH("nir_cosine_bcast_f32");
    return 0;
}

extern "C" int nir_cosine_bcast_bwd_f32(const float* q, const float* d, const float* g, int64_t B, int N, int D, float* dq, float* dd,
                                        nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(q && d && g && dq && dd && B >= 0 && N > 0 && D > 0 && D <= 512, "cosine_bcast_bwd: bad args (D <= 512)");
    if (B == 0) return 0;
    hipLaunchKernelGGL(cosine_bcast_bwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, q, d, g, B, N, D, dq, dd);
    NIR_CHECK_LAUNCH("nir_cosine_bcast_bwd_f32");
    return 0;
}

extern "C" int nir_rank_loss_softmax_nll_bwd(const float* scores, const float* labels, const float* grad_out, int64_t rows, int n, float* dscores,
                                             nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(scores && labels && grad_out && dscores && rows > 0 && n > 0, "rank_loss_softmax_nll_bwd: bad args");
    hipLaunchKernelGGL(softmax_nll_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, scores, labels, grad_out, rows,
                       n, dscores);
    NIR_CHECK_LAUNCH("nir_rank_loss_softmax_nll_bwd");
    return 0;
}
