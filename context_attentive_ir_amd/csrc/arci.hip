// ARC-I ranker (neuroir/rankers/arci.py:26-58, 60-105): per tower a stack of Conv1d(k, padding k/2) -> ReLU -> MaxPool1d(p), then
// mlp = Linear(inp, inp/2) -> Linear(inp/2, 1) over [query features, document features] (channel-major flatten, index f * feats + t).
//
// One kernel per layer, query and document rows in the same launch (the block index selects the tower):
//   conv1d_pool_split_kernel   64 conv positions x 128 filters per workgroup.  The rows of a tile are the positions of 64 / p CONSECUTIVE
//                              POOLED WINDOWS of the flattened [M, L / p] window list, so a pool window never straddles a tile (whatever p
//                              is) and the trailing L % p positions of a sequence are never computed (MaxPool1d's floor).  A row (m, t) and
//                              tap j read row t + j - k/2 of sequence m -- a table row gathered by id at layer 0, a row of the dense
//                              position-major [M, L, C] activation afterwards -- or zeros outside [0, L): the conv's own padding, which is
//                              not the PAD row of the table.  K runs tap-major over k * roundup(C, 32); every 32-wide step is staged through
//                              LDS as two fp16 terms (split2.hpp) and multiplied with the pre-split weight fragments by three
//                              v_mfma_f32_16x16x32_f16.  Epilogue through LDS: max over the p rows of a window, + bias, activation, then
//                              either the [M, L / p, F] store or the folded head: the pooled value times w_eff[f * feats + t], summed over
//                              64 filters by one wave in a fixed order -> partial [window][128-filter block][2].
//   conv1d_pool_f32_kernel     the same operation in plain fp32 FMA, one pooled window per workgroup: the path of a layer whose operands
//                              are not known to be below 2^15 (the pack-time bound, rankers/arci.py).  Slow, exact-fp32 class.
//   arci_finish_kernel         one wave per (query, candidate): the partials of the query and of the document in a fixed order, + b_eff.
// No float atomics anywhere: two calls give the same bits.
// The tile constants, the staging helpers and the declarations ARC-II's first stage uses (arcii.hip) are in conv_pool.hpp.
#include "conv_pool.hpp"
#include <algorithm>

namespace nir {

// Weight [F][C][k] (Conv1d layout) -> (a) split2 fragments: step ks covers K indices kk = 32 ks .. + 31 of the tap-major order
// kk = j * roundup(C, 32) + c; fragment (ks, nt, term) is 64 lanes x 8 halfs, lane l holding filter 16 nt + (l & 15), kk = 32 ks + 8 (l >> 4) + e
// (zeros for c >= C, filter >= F); (b) wt[(j C + c) F + f], fp32.  |w| >= 2^15 (or NaN) raises bit 1 of *flag.
__global__ __launch_bounds__(256) void conv1d_pack_kernel(const float* w, int C, int F, int k, uint4* planes, float* wt, int* flag) {
    const int Cp = (C + 31) & ~31, KS = k * (Cp >> 5), NT = (F + 15) >> 4;
    const int64_t nfrag = (int64_t)KS * NT * 64, total = (int64_t)gridDim.x * 256;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nfrag; i += total) {
        const int lane = (int)(i & 63);
        const int64_t tile = i >> 6;
        const int nt = (int)(tile % NT), ks = (int)(tile / NT);
        const int f = nt * 16 + (lane & 15);
        union { _Float16 h[8]; uint4 u; } hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int kk = ks * 32 + (lane >> 4) * 8 + e;
            const int j = kk / Cp, c = kk % Cp;
            const float v = (c < C && f < F) ? w[((int64_t)f * C + c) * k + j] : 0.f;
            bad |= !(fabsf(v) < 32768.f);
            hi.h[e] = split2_hi1_rne(v);
            lo.h[e] = split2_lo1(v, hi.h[e]);
        }
        planes[tile * 128 + lane] = hi.u;
        planes[tile * 128 + 64 + lane] = lo.u;
    }
    const int64_t nw = (int64_t)F * C * k;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nw; i += total) {
        const int j = (int)(i % k);
        const int c = (int)((i / k) % C);
        const int f = (int)(i / ((int64_t)k * C));
        wt[((int64_t)j * C + c) * F + f] = w[i];
    }
    if (bad) atomicOr(flag, 2);
}

__global__ __launch_bounds__(256) void conv1d_pool_split_kernel(ConvArgs a) {
    __shared__ uint4 smem[CV_ROWS * CV_EP_LD / 4];           // staging: 2 buffers x 2 terms x 64 rows x 64 bytes (16 KiB); epilogue: 64 x 132 floats
    const bool second = (int64_t)blockIdx.x >= a.nblk0;
    const ConvSide& s = second ? a.s[1] : a.s[0];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, F = a.F, k = a.k, p = a.p;
    const int Cp = (C + 31) & ~31, CB = Cp >> 5, KS = k * CB, NT = (F + 15) >> 4, NCB = (F + CV_COLS - 1) / CV_COLS;
    const int L = s.L, Lp = L / p, TW = CV_ROWS / p;
    const int64_t G = s.M * Lp;
    const int64_t bid = (int64_t)blockIdx.x - (second ? a.nblk0 : 0);
    const int cb = (int)(bid % NCB);
    const int64_t g0 = (bid / NCB) * TW;
    const int64_t* ids = s.ids;
    const float* xs = s.x;

    // staging role: thread -> (tile row, 8-channel chunk); the row's sequence and position are fixed for the whole K loop
    const int srow = tid >> 2, chunk = tid & 3;
    const int sw = srow / p;
    const bool rvalid = sw < TW && g0 + sw < G;
    int64_t m = 0;
    int t = 0;
    if (rvalid) {
        const int64_t g = g0 + sw;
        m = g / Lp;
        t = (int)(g % Lp) * p + srow % p;
    }
    const bool vec4 = (C & 3) == 0;
    auto src_of = [&](int j) -> const float* {
        const int ts = t + j - (k >> 1);
        if (!rvalid || ts < 0 || ts >= L) return nullptr;               // the conv's zero padding
        const int64_t r = m * L + ts;
        return xs + (ids ? ids[r] : r) * (int64_t)C;
    };
    auto stage = [&](int buf, const float (&v)[8]) {
        const Split2x4 lo4 = split2(make_float4(v[0], v[1], v[2], v[3])), hi4 = split2(make_float4(v[4], v[5], v[6], v[7]));
        smem[cv_slot(buf, 0, srow, chunk)] = make_uint4(lo4.hi.x, lo4.hi.y, hi4.hi.x, hi4.hi.y);
        smem[cv_slot(buf, 1, srow, chunk)] = make_uint4(lo4.lo.x, lo4.lo.y, hi4.lo.x, hi4.lo.y);
    };
    // MFMA role: wave -> column tiles nt0, nt0 + 1 of this block's 128 filters, all four row tiles
    const int nt0 = cb * (CV_COLS / 16) + wave * CV_CT;
    bool has[CV_CT];
#pragma unroll
    for (int j = 0; j < CV_CT; ++j) has[j] = nt0 + j < NT;
    auto load_w = [&](int ks, uint4 (&wv)[CV_CT][2]) {
#pragma unroll
        for (int j = 0; j < CV_CT; ++j) {
            if (has[j]) {
                const uint4* wp = s.planes + ((int64_t)ks * NT + nt0 + j) * 128 + lane;
                wv[j][0] = wp[0], wv[j][1] = wp[64];
            } else {
                wv[j][0] = wv[j][1] = make_uint4(0, 0, 0, 0);
            }
        }
    };

    f32x4 acc[CV_CT][CV_RT], acx[CV_CT][CV_RT];
#pragma unroll
    for (int j = 0; j < CV_CT; ++j)
#pragma unroll
        for (int i = 0; i < CV_RT; ++i) acc[j][i] = acx[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    float v[8];
    const float* cur = src_of(0);
    const float* nxt = k > 1 ? src_of(1) : nullptr;
    cv_load8(cur, chunk * 8, C, vec4, v);
    stage(0, v);
    uint4 wc[CV_CT][2];
    load_w(0, wc);
    __syncthreads();
    int tap = 0, cblk = 0;
    for (int ks = 0; ks < KS; ++ks) {
        const int buf = ks & 1;
        int ntap = tap, ncblk = cblk + 1;
        if (ncblk == CB) ncblk = 0, ntap = tap + 1;
        const bool more = ks + 1 < KS;
        uint4 wn[CV_CT][2];
        if (more) {                                // the next step's operands are in flight under this step's MFMAs
            if (ncblk == 0) {
                cur = nxt;
                nxt = ntap + 1 < k ? src_of(ntap + 1) : nullptr;
            }
            cv_load8(cur, ncblk * 32 + chunk * 8, C, vec4, v);
            load_w(ks + 1, wn);
        }
        f16x8 af[CV_RT][2];
#pragma unroll
        for (int i = 0; i < CV_RT; ++i) {
            af[i][0] = __builtin_bit_cast(f16x8, smem[cv_slot(buf, 0, 16 * i + (lane & 15), lane >> 4)]);
            af[i][1] = __builtin_bit_cast(f16x8, smem[cv_slot(buf, 1, 16 * i + (lane & 15), lane >> 4)]);
        }
#pragma unroll
        for (int j = 0; j < CV_CT; ++j) {
            if (has[j]) {
                const f16x8 w1 = __builtin_bit_cast(f16x8, wc[j][0]), w2 = __builtin_bit_cast(f16x8, wc[j][1]);
#pragma unroll
                for (int i = 0; i < CV_RT; ++i) {
                    acx[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][1], w1, acx[j][i], 0, 0, 0);
                    acx[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][0], w2, acx[j][i], 0, 0, 0);
                    acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][0], w1, acc[j][i], 0, 0, 0);
                }
            }
        }
        if (more) {
            stage(buf ^ 1, v);
#pragma unroll
            for (int j = 0; j < CV_CT; ++j) wc[j][0] = wn[j][0], wc[j][1] = wn[j][1];
        }
        __syncthreads();
        tap = ntap, cblk = ncblk;
    }

    // epilogue: the tile as fp32 in LDS (C / D layout: column lane & 15, rows 4 (lane >> 4) + r), then window by window
    float* ep = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int j = 0; j < CV_CT; ++j)
#pragma unroll
        for (int i = 0; i < CV_RT; ++i) {
            const f32x4 r4 = split2_combine(acc[j][i], acx[j][i]);
#pragma unroll
            for (int r = 0; r < 4; ++r) ep[(16 * i + 4 * (lane >> 4) + r) * CV_EP_LD + wave * (16 * CV_CT) + 16 * j + (lane & 15)] = r4[r];
        }
    __syncthreads();
    const int nwin = (int)(G - g0 < TW ? G - g0 : TW);
    for (int w0 = 0; w0 < nwin; w0 += 2) {
        const int w = w0 + (tid >> 7), col = tid & (CV_COLS - 1);       // (wave-uniform window; a wave covers 64 of its filters)
        if (w >= nwin) break;
        const int f = cb * CV_COLS + col;
        const int64_t g = g0 + w;
        float val = 0.f;
        if (f < F) {
            val = ep[(w * p) * CV_EP_LD + col];
            for (int r = 1; r < p; ++r) val = fmaxf(val, ep[(w * p + r) * CV_EP_LD + col]);
            val += s.bias[f];                     // (x -> x + b and ReLU are monotone: the max commutes with them bit for bit)
            if (a.act == NIR_ACT_RELU) val = fmaxf(val, 0.f);
        }
        if (!s.head_w) {
            if (f < F) s.out[g * F + f] = val;
        } else {
            const float part = wave_sum(f < F ? val * s.head_w[(int64_t)f * Lp + (int)(g % Lp)] : 0.f);
            if (lane == 0) s.out[(g * NCB + cb) * 2 + (wave & 1)] = part;
        }
    }
}

// One pooled window per workgroup, thread f, f + 256, ..: fp32 FMA over the k C products of each of the p positions.
__global__ __launch_bounds__(256) void conv1d_pool_f32_kernel(ConvArgs a) {
    __shared__ float red[4];
    const bool second = (int64_t)blockIdx.x >= a.nblk0;
    const ConvSide& s = second ? a.s[1] : a.s[0];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, F = a.F, k = a.k, p = a.p, NCB = (F + CV_COLS - 1) / CV_COLS;
    const int L = s.L, Lp = L / p;
    const int64_t g = (int64_t)blockIdx.x - (second ? a.nblk0 : 0);
    const int64_t m = g / Lp;
    const int tp = (int)(g % Lp);
    float part = 0.f;
    for (int f = tid; f < F; f += 256) {
        float mx = -INFINITY;
        for (int r = 0; r < p; ++r) {
            float acc = 0.f;
            for (int j = 0; j < k; ++j) {
                const int ts = tp * p + r + j - (k >> 1);
                if (ts < 0 || ts >= L) continue;
                const int64_t row = m * L + ts;
                const float* src = s.x + (s.ids ? s.ids[row] : row) * (int64_t)C;
                const float* wj = s.wt + (int64_t)j * C * F + f;
                for (int c = 0; c < C; ++c) acc = fmaf(src[c], wj[(int64_t)c * F], acc);
            }
            mx = fmaxf(mx, acc);
        }
        mx += s.bias[f];
        if (a.act == NIR_ACT_RELU) mx = fmaxf(mx, 0.f);
        if (!s.head_w) s.out[g * F + f] = mx;
        else part = fmaf(mx, s.head_w[(int64_t)f * Lp + tp], part);
    }
    if (s.head_w) {
        part = wave_sum(part);
        if (lane == 0) red[wave] = part;
        __syncthreads();
        for (int i = tid; i < NCB * 2; i += 256) s.out[g * NCB * 2 + i] = i == 0 ? (red[0] + red[1]) + (red[2] + red[3]) : 0.f;
    }
}

// scores[b][n] = sum of the nq partials of query b + sum of the nd partials of document (b, n) + b_eff; one wave per pair, fixed order
__global__ __launch_bounds__(256) void arci_finish_kernel(const float* qpart, int nq, const float* dpart, int nd, const float* head_b, int64_t B, int N,
                                                          float* scores) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= B * N) return;
    const int64_t b = pair / N;
    float sq = 0.f, sd = 0.f;
    for (int i = lane; i < nq; i += 64) sq += qpart[b * nq + i];
    for (int i = lane; i < nd; i += 64) sd += dpart[pair * nd + i];
    const float tot = wave_sum(sq) + wave_sum(sd);
    if (lane == 0) scores[pair] = tot + head_b[0];
}

int conv_check(const nir_conv1d_layer* ly, const char* who) {
    NIR_REQUIRE(ly, "%s: null layer", who);
    NIR_REQUIRE(ly->C_in >= 1 && ly->C_in <= CV_MAX_C, "%s: C_in %d unsupported (1 <= C_in <= %d)", who, ly->C_in, CV_MAX_C);
    NIR_REQUIRE(ly->F >= 1 && ly->F <= CV_MAX_F, "%s: F %d unsupported (1 <= F <= %d)", who, ly->F, CV_MAX_F);
    NIR_REQUIRE(ly->k >= 1 && ly->k <= CV_MAX_K && (ly->k & 1), "%s: kernel size %d unsupported (odd, <= %d)", who, ly->k, CV_MAX_K);
    NIR_REQUIRE(ly->p >= 1 && ly->p <= CV_MAX_P, "%s: pool size %d unsupported (1 <= p <= %d)", who, ly->p, CV_MAX_P);
    NIR_REQUIRE(ly->path == NIR_CONV1D_SPLIT || ly->path == NIR_CONV1D_FP32, "%s: path %d unknown", who, ly->path);
    NIR_REQUIRE(ly->bias && (ly->path == NIR_CONV1D_SPLIT ? (const void*)ly->planes : (const void*)ly->wt), "%s: null weight", who);
    return 0;
}

// both sides share (C, F, k, p); a side with M == 0 contributes no block
int conv_launch(ConvSide s0, ConvSide s1, int C, int F, int k, int p, int act, int path, hipStream_t st, const char* who) {
    ConvArgs a;
    a.s[0] = s0, a.s[1] = s1;
    a.C = C, a.F = F, a.k = k, a.p = p, a.act = act;
    int64_t nb[2];
    for (int i = 0; i < 2; ++i) {
        const int64_t G = a.s[i].M * (a.s[i].L / p);
        nb[i] = path == NIR_CONV1D_SPLIT ? (G + CV_ROWS / p - 1) / (CV_ROWS / p) * (int64_t)conv_ncb(F) : G;
    }
    a.nblk0 = nb[0];
    NIR_REQUIRE(nb[0] + nb[1] < ((int64_t)1 << 31), "%s: too many rows for one launch", who);
    if (nb[0] + nb[1] == 0) return 0;
    if (path == NIR_CONV1D_SPLIT) {
        ProfScope ps(prof_shape_name("conv1d_pool_split_kernel", (s0.M * (s0.L / p) + s1.M * (s1.L / p)) * p, F, (long long)k * C), st);
        hipLaunchKernelGGL(conv1d_pool_split_kernel, dim3((unsigned)(nb[0] + nb[1])), dim3(256), 0, st, a);
    } else {
        ProfScope ps("conv1d_pool_f32_kernel", st);
        hipLaunchKernelGGL(conv1d_pool_f32_kernel, dim3((unsigned)(nb[0] + nb[1])), dim3(256), 0, st, a);
    }
    NIR_CHECK_LAUNCH(who);
    return 0;
}

ConvSide conv_side(const int64_t* ids, const float* x, const nir_conv1d_layer* ly, const float* head_w, float* out, int64_t M, int L) {
    return ConvSide{ids, x, (const uint4*)ly->planes, ly->wt, ly->bias, head_w, out, M, L};
}

int conv_pack_launch(const float* w, int C, int F, int taps, void* planes, float* wt, int* flag, hipStream_t st, const char* who) {
    const int64_t n = (int64_t)taps * ((C + 31) / 32) * ((F + 15) / 16) * 64;
    hipLaunchKernelGGL(conv1d_pack_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, w, C, F, taps, (uint4*)planes, wt, flag);
    NIR_CHECK_LAUNCH(who);
    return 0;
}

}  // namespace nir

extern "C" size_t nir_conv1d_planes_bytes(int C_in, int F, int k) {
    if (C_in < 1 || F < 1 || k < 1) return 0;
    return (size_t)k * ((C_in + 31) / 32) * ((F + 15) / 16) * 2 * 64 * 16;
}

extern "C" int nir_conv1d_pack(const float* w, int C_in, int F, int k, void* planes, float* wt, int* flag, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(w && planes && wt && flag, "conv1d_pack: null pointer");
    NIR_REQUIRE(C_in >= 1 && C_in <= CV_MAX_C && F >= 1 && F <= CV_MAX_F && k >= 1 && k <= CV_MAX_K && (k & 1),
                "conv1d_pack: C_in %d / F %d / k %d unsupported (C_in <= %d, F <= %d, k odd <= %d)", C_in, F, k, CV_MAX_C, CV_MAX_F, CV_MAX_K);
    return conv_pack_launch(w, C_in, F, k, planes, wt, flag, (hipStream_t)stream, "nir_conv1d_pack");
}

extern "C" size_t nir_conv1d_pool_out_floats(int64_t M, int L, int F, int p, int head) {
    if (M < 0 || L < 1 || F < 1 || p < 1) return 0;
    return (size_t)M * (L / p) * (head ? nir::conv_ncb(F) * 2 : (size_t)F);
}

extern "C" int nir_conv1d_pool_f32(const int64_t* ids, const float* x, int64_t M, int L, const nir_conv1d_layer* layer, int act, const float* head_w,
                                   float* out, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(x && out, "conv1d_pool: null pointer");
    NIR_PROPAGATE(conv_check(layer, "conv1d_pool"));
    NIR_REQUIRE(M >= 0 && L >= 1, "conv1d_pool: bad dims M=%lld L=%d", (long long)M, L);
    NIR_REQUIRE(act == NIR_ACT_NONE || act == NIR_ACT_RELU, "conv1d_pool: act %d unsupported (none, relu)", act);
    return conv_launch(conv_side(ids, x, layer, head_w, out, M, L), ConvSide{}, layer->C_in, layer->F, layer->k, layer->p, act, layer->path,
                       (hipStream_t)stream, "nir_conv1d_pool_f32");
}

// pooled width of every layer; false when one of them is 0
static bool arci_widths(const nir_arci_weights* w, int L, int* out) {
    for (int i = 0; i < w->n_layers; ++i) {
        L /= w->q[i].p;
        if (L == 0) return false;
        out[i] = L;
    }
    return true;
}

static int arci_check(const nir_arci_weights* w, int QL, int DL, int E, int* lq, int* ld) {
    using namespace nir;
    NIR_REQUIRE(w, "arci: null weights");
    NIR_REQUIRE(w->n_layers >= 1 && w->n_layers <= NIR_ARCI_MAX_LAYERS, "arci: %d layers unsupported (1 .. %d)", w->n_layers, NIR_ARCI_MAX_LAYERS);
    NIR_REQUIRE(w->head_wq && w->head_wd && w->head_b, "arci: null head");
    for (int i = 0; i < w->n_layers; ++i) {
        NIR_PROPAGATE(conv_check(&w->q[i], "arci (query tower)"));
        NIR_PROPAGATE(conv_check(&w->d[i], "arci (document tower)"));
        NIR_REQUIRE(w->q[i].C_in == w->d[i].C_in && w->q[i].F == w->d[i].F && w->q[i].k == w->d[i].k && w->q[i].p == w->d[i].p,
                    "arci: layer %d differs between the towers", i);
        NIR_REQUIRE(w->q[i].C_in == (i == 0 ? E : w->q[i - 1].F), "arci: layer %d reads %d channels, its input has %d", i, w->q[i].C_in,
                    i == 0 ? E : w->q[i - 1].F);
    }
    NIR_REQUIRE(QL >= 1 && DL >= 1 && arci_widths(w, QL, lq) && arci_widths(w, DL, ld) && lq[w->n_layers - 1] == w->q_feats &&
                    ld[w->n_layers - 1] == w->d_feats,
                "arci: widths %d / %d do not pool to the %d / %d positions the head was built for (arci.py:53-58)", QL, DL, w->q_feats, w->d_feats);
    return 0;
}

extern "C" size_t nir_arci_workspace_bytes(int B, int N, int QL, int DL, const nir_arci_weights* w) {
    using namespace nir;
    int lq[NIR_ARCI_MAX_LAYERS], ld[NIR_ARCI_MAX_LAYERS];
    if (!w || w->n_layers < 1 || w->n_layers > NIR_ARCI_MAX_LAYERS || B < 0 || N < 1 || QL < 1 || DL < 1) return 0;
    for (int i = 0; i < w->n_layers; ++i)
        if (w->q[i].p < 1 || w->q[i].F < 1) return 0;
    if (!arci_widths(w, QL, lq) || !arci_widths(w, DL, ld)) return 0;
    size_t tot = 0;
    const size_t M = (size_t)B * N;
    for (int i = 0; i < w->n_layers; ++i) {
        const size_t per = i + 1 < w->n_layers ? (size_t)w->q[i].F : conv_ncb(w->q[i].F) * 2;
        tot += align_up((size_t)B * lq[i] * per * 4, 256) + align_up(M * ld[i] * per * 4, 256);
    }
    return tot;
}

extern "C" int nir_arci_score(const int64_t* q_ids, const int64_t* d_ids, int B, int N, int QL, int DL, const float* table, int64_t V, int E,
                              const nir_arci_weights* w, void* workspace, size_t workspace_bytes, float* scores, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(q_ids && d_ids && table && scores, "arci: null pointer");
    NIR_REQUIRE(B >= 0 && N > 0 && V > 0 && E > 0, "arci: bad dims B=%d N=%d V=%lld E=%d", B, N, (long long)V, E);
    int lq[NIR_ARCI_MAX_LAYERS], ld[NIR_ARCI_MAX_LAYERS];
    NIR_PROPAGATE(arci_check(w, QL, DL, E, lq, ld));
    if (B == 0) return 0;
    const int nl = w->n_layers;
    const int64_t M = (int64_t)B * N;
    Workspace ws(workspace, workspace_bytes);
    float *oq[NIR_ARCI_MAX_LAYERS], *od[NIR_ARCI_MAX_LAYERS];
    for (int i = 0; i < nl; ++i) {
        const size_t per = i + 1 < nl ? (size_t)w->q[i].F : conv_ncb(w->q[i].F) * 2;
        oq[i] = ws.take<float>((size_t)B * lq[i] * per);
        od[i] = ws.take<float>((size_t)M * ld[i] * per);
    }
    NIR_REQUIRE(ws.ok(), "arci: workspace too small (%zu < %zu bytes)", workspace_bytes, ws.off);
    for (int i = 0; i < nl; ++i) {
        const bool last = i + 1 == nl;
        const nir_conv1d_layer *q = &w->q[i], *d = &w->d[i];
        const ConvSide sq = conv_side(i == 0 ? q_ids : nullptr, i == 0 ? table : oq[i - 1], q, last ? w->head_wq : nullptr, oq[i], B, i == 0 ? QL : lq[i - 1]);
        const ConvSide sd = conv_side(i == 0 ? d_ids : nullptr, i == 0 ? table : od[i - 1], d, last ? w->head_wd : nullptr, od[i], M, i == 0 ? DL : ld[i - 1]);
        // one launch per layer: the split path only when both towers' operands are bounded
        const int path = (q->path == NIR_CONV1D_SPLIT && d->path == NIR_CONV1D_SPLIT) ? NIR_CONV1D_SPLIT : NIR_CONV1D_FP32;
        NIR_REQUIRE(path == NIR_CONV1D_SPLIT || (q->wt && d->wt), "arci: layer %d has no fp32 weights", i);
        NIR_PROPAGATE(conv_launch(sq, sd, q->C_in, q->F, q->k, q->p, NIR_ACT_RELU, path, (hipStream_t)stream, "nir_arci_score (layer)"));
    }
    {
        const int per = (int)conv_ncb(w->q[nl - 1].F) * 2;
        ProfScope ps("arci_finish_kernel", (hipStream_t)stream);
        hipLaunchKernelGGL(arci_finish_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, oq[nl - 1], lq[nl - 1] * per, od[nl - 1],
                           ld[nl - 1] * per, w->head_b, (int64_t)B, N, scores);
        NIR_CHECK_LAUNCH("nir_arci_score (finish)");
    }
    return 0;
}
