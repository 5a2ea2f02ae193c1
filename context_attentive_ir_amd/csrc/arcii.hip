// ARC-II ranker (neuroir/rankers/arcii.py:11-56 construction, :58-111 forward): Eq = conv_query(embed(q)) [B, F1, QL] and
// Ed = conv_doc(embed(d)) [B N, F1, DL] (no activation), the grid X[m, f, i, j] = Ed[m, f, i] + Eq[m / N, f, j] (document axis first) through
// MaxPool2d(2, 2), then per layer Conv2d(kh x kw, padding (kh/2, kw/2)) -> ReLU -> MaxPool2d(ph x pw), flatten(1), and
// mlp = Linear(inp, inp/2) -> Linear(inp/2, 1).
//
// The first pool is separable bit for bit (fp32 addition is monotone in each operand): max_pool2d(Ed + Eq, 2 x 2) ==
// max_pool1d(Ed, 2) + max_pool1d(Eq, 2).  So stage 1 is arci.hip's conv1d_pool kernel (act none, p 2, both towers in one launch) and the
// [B N, F1, DL, QL] grid is never formed.
//
//   conv2d_pool_split_kernel   the 2-D form of conv1d_pool_split_kernel: 64 conv positions x 128 filters per workgroup; the rows of a tile
//                              are the ph pw positions of 64 / (ph pw) CONSECUTIVE POOLED WINDOWS of the flattened [M, H/ph, W/pw] window
//                              list, so no window straddles a tile, floor-dropped rows and columns are never computed and tiles pack
//                              across pair ends.  Row (m, i, j), tap (a, b) reads position (i + a - kh/2, j + b - kw/2): a row of the
//                              dense [M, H, W, C] activation, or in the OUTER-SUM mode Pd[m, i', :] + Pq[m / N, j', :], added in fp32
//                              before the split -- and ZERO when i' or j' is outside the grid (the conv pads the grid, not its terms).
//                              K runs tap-major (row-major taps) over kh kw roundup(C, 32); staging, MFMAs and the epilogue are the
//                              1-D kernel's: max over the window's rows, + bias, activation, then the [M, H/ph, W/pw, F] store or the
//                              folded head, pooled . w_eff[f Hd Hq + i Hq + j] summed per wave in a fixed order -> [window][block][2].
//   conv2d_pool_f32_kernel     the same operation in plain fp32 FMA, one pooled window per workgroup (input bound >= 2^15).
//   arcii_finish_kernel        one wave per (query, candidate): its partials in a fixed order, + b_eff.
// No float atomics anywhere: two calls give the same bits.
#include "conv_pool.hpp"

namespace nir {

struct Conv2dArgs {
    const float* x;           // dense [M, H, W, C], or NULL: the outer sum of
    const float* pd;          //   [M, H, C]
    const float* pq;          //   [M / N, W, C]
    const uint4* planes;
    const float* wt;          // fp32 [kh kw C][F]
    const float* bias;
    const float* head_w;      // NULL: out is [M, H/ph, W/pw, F]; else w_eff [F][H/ph][W/pw] and out is the partial list [windows][NCB][2]
    float* out;
    int64_t M;
    int N, H, W, C, F, kh, kw, ph, pw, act;
};

__global__ __launch_bounds__(256) void conv2d_pool_split_kernel(Conv2dArgs a) {
    __shared__ uint4 smem[CV_ROWS * CV_EP_LD / 4];           // staging: 2 buffers x 2 terms x 64 rows x 64 bytes (16 KiB); epilogue: 64 x 132 floats
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, F = a.F, kw = a.kw, H = a.H, W = a.W;
    const int Cp = (C + 31) & ~31, CB = Cp >> 5, KS = a.kh * kw * CB, NT = (F + 15) >> 4, NCB = (F + CV_COLS - 1) / CV_COLS;
    const int P = a.ph * a.pw, Hp = H / a.ph, Wp = W / a.pw, HW = Hp * Wp, TW = CV_ROWS / P;
    const int64_t G = a.M * HW;
    const int64_t bid = blockIdx.x;
    const int cb = (int)(bid % NCB);
    const int64_t g0 = (bid / NCB) * TW;

    // staging role: thread -> (tile row, 8-channel chunk); the row's pair and grid position are fixed for the whole K loop
    const int srow = tid >> 2, chunk = tid & 3;
    const int sw = srow / P;
    const bool rvalid = sw < TW && g0 + sw < G;
    int64_t m = 0;
    int ri = 0, rj = 0;
    if (rvalid) {
        const int64_t g = g0 + sw;
        const int rem = (int)(g % HW), r = srow % P;
        m = g / HW;
        ri = (rem / Wp) * a.ph + r / a.pw;
        rj = (rem % Wp) * a.pw + r % a.pw;
    }
    const int64_t mq = m / a.N;
    const bool vec4 = (C & 3) == 0;
    const float *s0 = nullptr, *s1 = nullptr;      // the tap's source rows: dense (s0), or the document and the query term (s0, s1); both NULL = zero
    auto set_tap = [&](int ta, int tb) {
        const int i2 = ri + ta - (a.kh >> 1), j2 = rj + tb - (kw >> 1);
        s0 = s1 = nullptr;
        if (!rvalid || i2 < 0 || i2 >= H || j2 < 0 || j2 >= W) return;              // the conv's zero padding of the GRID
        if (a.x) {
            s0 = a.x + ((m * H + i2) * W + j2) * (int64_t)C;
        } else {
            s0 = a.pd + (m * H + i2) * (int64_t)C;
            s1 = a.pq + (mq * W + j2) * (int64_t)C;
        }
    };
    auto load = [&](int c, float (&v)[8]) {
        cv_load8(s0, c, C, vec4, v);
        if (s1) {
            float u[8];
            cv_load8(s1, c, C, vec4, u);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += u[e];
        }
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
                const uint4* wp = a.planes + ((int64_t)ks * NT + nt0 + j) * 128 + lane;
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
    int ta = 0, tb = 0, cblk = 0;
    set_tap(0, 0);
    load(chunk * 8, v);
    stage(0, v);
    uint4 wc[CV_CT][2];
    load_w(0, wc);
    __syncthreads();
    for (int ks = 0; ks < KS; ++ks) {
        const int buf = ks & 1;
        const bool more = ks + 1 < KS;
        uint4 wn[CV_CT][2];
        if (more) {                                // the next step's operands are in flight under this step's MFMAs
            if (++cblk == CB) {
                cblk = 0;
                if (++tb == kw) tb = 0, ++ta;
                set_tap(ta, tb);
            }
            load(cblk * 32 + chunk * 8, v);
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
            val = ep[(w * P) * CV_EP_LD + col];
            for (int r = 1; r < P; ++r) val = fmaxf(val, ep[(w * P + r) * CV_EP_LD + col]);
            val += a.bias[f];                     // (x -> x + b and ReLU are monotone: the max commutes with them bit for bit)
            if (a.act == NIR_ACT_RELU) val = fmaxf(val, 0.f);
        }
        if (!a.head_w) {
            if (f < F) a.out[g * F + f] = val;
        } else {
            const float part = wave_sum(f < F ? val * a.head_w[(int64_t)f * HW + (int)(g % HW)] : 0.f);      // g % HW = i Hq + j
            if (lane == 0) a.out[(g * NCB + cb) * 2 + (wave & 1)] = part;
        }
    }
}

// One pooled window per workgroup, thread f, f + 256, ..: fp32 FMA over the kh kw C products of each of the ph pw positions.
__global__ __launch_bounds__(256) void conv2d_pool_f32_kernel(Conv2dArgs a) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, F = a.F, H = a.H, W = a.W, NCB = (F + CV_COLS - 1) / CV_COLS;
    const int P = a.ph * a.pw, Hp = H / a.ph, Wp = W / a.pw, HW = Hp * Wp;
    const int64_t g = blockIdx.x;
    const int64_t m = g / HW, mq = m / a.N;
    const int rem = (int)(g % HW), ip = rem / Wp, jp = rem % Wp;
    float part = 0.f;
    for (int f = tid; f < F; f += 256) {
        float mx = -INFINITY;
        for (int r = 0; r < P; ++r) {
            const int i = ip * a.ph + r / a.pw, j = jp * a.pw + r % a.pw;
            float acc = 0.f;
            for (int t = 0; t < a.kh * a.kw; ++t) {
                const int i2 = i + t / a.kw - (a.kh >> 1), j2 = j + t % a.kw - (a.kw >> 1);
                if (i2 < 0 || i2 >= H || j2 < 0 || j2 >= W) continue;
                const float* wj = a.wt + (int64_t)t * C * F + f;
                if (a.x) {
                    const float* src = a.x + ((m * H + i2) * W + j2) * (int64_t)C;
                    for (int c = 0; c < C; ++c) acc = fmaf(src[c], wj[(int64_t)c * F], acc);
                } else {
                    const float *sd = a.pd + (m * H + i2) * (int64_t)C, *sq = a.pq + (mq * W + j2) * (int64_t)C;
                    for (int c = 0; c < C; ++c) acc = fmaf(sd[c] + sq[c], wj[(int64_t)c * F], acc);
                }
            }
            mx = fmaxf(mx, acc);
        }
        mx += a.bias[f];
        if (a.act == NIR_ACT_RELU) mx = fmaxf(mx, 0.f);
        if (!a.head_w) a.out[g * F + f] = mx;
        else part = fmaf(mx, a.head_w[(int64_t)f * HW + rem], part);
    }
    if (a.head_w) {
        part = wave_sum(part);
        if (lane == 0) red[wave] = part;
        __syncthreads();
        for (int i = tid; i < NCB * 2; i += 256) a.out[g * NCB * 2 + i] = i == 0 ? (red[0] + red[1]) + (red[2] + red[3]) : 0.f;
    }
}

// scores[pair] = sum of the pair's n partials + b_eff; one wave per pair, fixed order
__global__ __launch_bounds__(256) void arcii_finish_kernel(const float* part, int n, const float* head_b, int64_t pairs, float* scores) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= pairs) return;
    float s = 0.f;
    for (int i = lane; i < n; i += 64) s += part[pair * n + i];
    const float tot = wave_sum(s);
    if (lane == 0) scores[pair] = tot + head_b[0];
}

static bool conv2d_kernel_ok(int k) { return k >= 1 && k <= CV_MAX_K && (k & 1); }

static int conv2d_check(const nir_conv2d_layer* ly, const char* who) {
    NIR_REQUIRE(ly, "%s: null layer", who);
    NIR_REQUIRE(ly->C_in >= 1 && ly->C_in <= CV_MAX_C, "%s: C_in %d unsupported (1 <= C_in <= %d)", who, ly->C_in, CV_MAX_C);
    NIR_REQUIRE(ly->F >= 1 && ly->F <= CV_MAX_F, "%s: F %d unsupported (1 <= F <= %d)", who, ly->F, CV_MAX_F);
    NIR_REQUIRE(conv2d_kernel_ok(ly->kh) && conv2d_kernel_ok(ly->kw), "%s: kernel size %d x %d unsupported (odd, <= %d)", who, ly->kh, ly->kw,
                CV_MAX_K);
    NIR_REQUIRE(ly->ph >= 1 && ly->pw >= 1 && (int64_t)ly->ph * ly->pw <= CV_MAX_P, "%s: pool size %d x %d unsupported (1 <= ph pw <= %d)", who,
                ly->ph, ly->pw, CV_MAX_P);
    NIR_REQUIRE(ly->path == NIR_CONV1D_SPLIT || ly->path == NIR_CONV1D_FP32, "%s: path %d unknown", who, ly->path);
    NIR_REQUIRE(ly->bias && (ly->path == NIR_CONV1D_SPLIT ? (const void*)ly->planes : (const void*)ly->wt), "%s: null weight", who);
    return 0;
}

// the layer is checked; H, W >= 1; a grid that pools to nothing launches nothing
static int conv2d_launch(const float* x, const float* pd, const float* pq, int64_t M, int N, int H, int W, const nir_conv2d_layer* ly, int act,
                         const float* head_w, float* out, hipStream_t st, const char* who) {
    Conv2dArgs a{x, pd, pq, (const uint4*)ly->planes, ly->wt, ly->bias, head_w, out, M, N, H, W, ly->C_in, ly->F, ly->kh, ly->kw, ly->ph, ly->pw, act};
    const int P = ly->ph * ly->pw;
    const int64_t G = M * (H / ly->ph) * (W / ly->pw);
    const int64_t nb = ly->path == NIR_CONV1D_SPLIT ? (G + CV_ROWS / P - 1) / (CV_ROWS / P) * (int64_t)conv_ncb(ly->F) : G;
    NIR_REQUIRE(nb < ((int64_t)1 << 31), "%s: too many rows for one launch", who);
    if (nb == 0) return 0;
    if (ly->path == NIR_CONV1D_SPLIT) {
        ProfScope ps(prof_shape_name("conv2d_pool_split_kernel", G * P, ly->F, (long long)ly->kh * ly->kw * ly->C_in), st);
        hipLaunchKernelGGL(conv2d_pool_split_kernel, dim3((unsigned)nb), dim3(256), 0, st, a);
    } else {
        ProfScope ps("conv2d_pool_f32_kernel", st);
        hipLaunchKernelGGL(conv2d_pool_f32_kernel, dim3((unsigned)nb), dim3(256), 0, st, a);
    }
    NIR_CHECK_LAUNCH(who);
    return 0;
}

// the grid after every 2-D layer (hd[i] x hq[i]); false when a side pools to 0 anywhere
static bool arcii_grids(const nir_arcii_weights* w, int QL, int DL, int* hd, int* hq) {
    int d = DL / 2, q = QL / 2;
    if (d == 0 || q == 0) return false;
    for (int i = 0; i < w->n_layers; ++i) {
        d /= w->l[i].ph, q /= w->l[i].pw;
        if (d == 0 || q == 0) return false;
        hd[i] = d, hq[i] = q;
    }
    return true;
}

static int arcii_check(const nir_arcii_weights* w, int QL, int DL, int E, int* hd, int* hq) {
    NIR_REQUIRE(w, "arcii: null weights");
    NIR_REQUIRE(w->n_layers >= 1 && w->n_layers <= NIR_ARCII_MAX_LAYERS, "arcii: %d 2-D layers unsupported (1 .. %d)", w->n_layers,
                NIR_ARCII_MAX_LAYERS);
    NIR_REQUIRE(w->head_w && w->head_b, "arcii: null head");
    NIR_PROPAGATE(conv_check(&w->q, "arcii (conv_query)"));
    NIR_PROPAGATE(conv_check(&w->d, "arcii (conv_doc)"));
    NIR_REQUIRE(w->q.C_in == E && w->d.C_in == E && w->q.F == w->d.F && w->q.k == w->d.k && w->q.p == 2 && w->d.p == 2,
                "arcii: conv_query and conv_doc must read %d channels and share filters, kernel size and the pool of 2", E);
    for (int i = 0; i < w->n_layers; ++i) {
        NIR_PROPAGATE(conv2d_check(&w->l[i], "arcii (conv2d layer)"));
        const int cin = i == 0 ? w->q.F : w->l[i - 1].F;
        NIR_REQUIRE(w->l[i].C_in == cin, "arcii: 2-D layer %d reads %d channels, its input has %d", i, w->l[i].C_in, cin);
    }
    const int nl = w->n_layers;
    NIR_REQUIRE(QL >= 1 && DL >= 1 && arcii_grids(w, QL, DL, hd, hq) && (int64_t)w->l[nl - 1].F * hd[nl - 1] * hq[nl - 1] == w->feats,
                "arcii: widths %d / %d do not pool to the %d features the head was built for (arcii.py:108-110)", QL, DL, w->feats);
    return 0;
}

}  // namespace nir

extern "C" size_t nir_conv2d_planes_bytes(int C_in, int F, int kh, int kw) {
    if (C_in < 1 || F < 1 || kh < 1 || kw < 1) return 0;
    return (size_t)kh * kw * ((C_in + 31) / 32) * ((F + 15) / 16) * 2 * 64 * 16;
}

extern "C" int nir_conv2d_pack(const float* w, int C_in, int F, int kh, int kw, void* planes, float* wt, int* flag, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(w && planes && wt && flag, "conv2d_pack: null pointer");
    NIR_REQUIRE(C_in >= 1 && C_in <= CV_MAX_C && F >= 1 && F <= CV_MAX_F && conv2d_kernel_ok(kh) && conv2d_kernel_ok(kw),
                "conv2d_pack: C_in %d / F %d / kernel %d x %d unsupported (C_in <= %d, F <= %d, kernel sizes odd <= %d)", C_in, F, kh, kw, CV_MAX_C,
                CV_MAX_F, CV_MAX_K);
    return conv_pack_launch(w, C_in, F, kh * kw, planes, wt, flag, (hipStream_t)stream, "nir_conv2d_pack");
}

extern "C" size_t nir_conv2d_pool_out_floats(int64_t M, int H, int W, int F, int ph, int pw, int head) {
    if (M < 0 || H < 1 || W < 1 || F < 1 || ph < 1 || pw < 1) return 0;
    return (size_t)M * (H / ph) * (W / pw) * (head ? nir::conv_ncb(F) * 2 : (size_t)F);
}

extern "C" int nir_conv2d_pool_f32(const float* x, const float* pd, const float* pq, int64_t M, int N, int H, int W, const nir_conv2d_layer* layer,
                                   int act, const float* head_w, float* out, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(out && (x ? !pd && !pq : pd && pq), "conv2d_pool: give the dense input or both terms of the outer sum");
    NIR_PROPAGATE(conv2d_check(layer, "conv2d_pool"));
    NIR_REQUIRE(M >= 0 && H >= 1 && W >= 1, "conv2d_pool: bad dims M=%lld H=%d W=%d", (long long)M, H, W);
    NIR_REQUIRE(x ? N == 1 : (N >= 1 && M % N == 0), "conv2d_pool: N %d unsupported (1 with a dense input; a divisor of M = %lld with the outer sum)", N,
                (long long)M);
    NIR_REQUIRE(act == NIR_ACT_NONE || act == NIR_ACT_RELU, "conv2d_pool: act %d unsupported (none, relu)", act);
    return conv2d_launch(x, pd, pq, M, N, H, W, layer, act, head_w, out, (hipStream_t)stream, "nir_conv2d_pool_f32");
}

extern "C" size_t nir_arcii_workspace_bytes(int B, int N, int QL, int DL, const nir_arcii_weights* w) {
    using namespace nir;
    int hd[NIR_ARCII_MAX_LAYERS], hq[NIR_ARCII_MAX_LAYERS];
    if (!w || w->n_layers < 1 || w->n_layers > NIR_ARCII_MAX_LAYERS || B < 0 || N < 1 || QL < 1 || DL < 1 || w->q.F < 1) return 0;
    for (int i = 0; i < w->n_layers; ++i)
        if (w->l[i].ph < 1 || w->l[i].pw < 1 || w->l[i].F < 1) return 0;
    if (!arcii_grids(w, QL, DL, hd, hq)) return 0;
    const size_t M = (size_t)B * N;
    size_t tot = align_up((size_t)B * (QL / 2) * w->q.F * 4, 256) + align_up(M * (DL / 2) * w->q.F * 4, 256);
    for (int i = 0; i < w->n_layers; ++i) {
        const size_t per = i + 1 < w->n_layers ? (size_t)w->l[i].F : conv_ncb(w->l[i].F) * 2;
        tot += align_up(M * hd[i] * hq[i] * per * 4, 256);
    }
    return tot;
}

extern "C" int nir_arcii_score(const int64_t* q_ids, const int64_t* d_ids, int B, int N, int QL, int DL, const float* table, int64_t V, int E,
                               const nir_arcii_weights* w, void* workspace, size_t workspace_bytes, float* scores, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(q_ids && d_ids && table && scores, "arcii: null pointer");
    NIR_REQUIRE(B >= 0 && N > 0 && V > 0 && E > 0, "arcii: bad dims B=%d N=%d V=%lld E=%d", B, N, (long long)V, E);
    int hd[NIR_ARCII_MAX_LAYERS], hq[NIR_ARCII_MAX_LAYERS];
    NIR_PROPAGATE(arcii_check(w, QL, DL, E, hd, hq));
    if (B == 0) return 0;
    const int nl = w->n_layers, F1 = w->q.F;
    const int64_t M = (int64_t)B * N;
    hipStream_t st = (hipStream_t)stream;
    Workspace ws(workspace, workspace_bytes);
    float* pq = ws.take<float>((size_t)B * (QL / 2) * F1);
    float* pd = ws.take<float>((size_t)M * (DL / 2) * F1);
    float* o[NIR_ARCII_MAX_LAYERS];
    for (int i = 0; i < nl; ++i) o[i] = ws.take<float>((size_t)M * hd[i] * hq[i] * (i + 1 < nl ? (size_t)w->l[i].F : conv_ncb(w->l[i].F) * 2));
    NIR_REQUIRE(ws.ok(), "arcii: workspace too small (%zu < %zu bytes)", workspace_bytes, ws.off);
    {   // stage 1: both towers, no activation, the separable half of MaxPool2d(2, 2)
        const int path = (w->q.path == NIR_CONV1D_SPLIT && w->d.path == NIR_CONV1D_SPLIT) ? NIR_CONV1D_SPLIT : NIR_CONV1D_FP32;
        NIR_REQUIRE(path == NIR_CONV1D_SPLIT || (w->q.wt && w->d.wt), "arcii: the 1-D convolutions have no fp32 weights");
        NIR_PROPAGATE(conv_launch(conv_side(q_ids, table, &w->q, nullptr, pq, B, QL), conv_side(d_ids, table, &w->d, nullptr, pd, M, DL), E, F1, w->q.k, 2,
                                  NIR_ACT_NONE, path, st, "nir_arcii_score (1-D stage)"));
    }
    for (int i = 0; i < nl; ++i) {
        const float* hw = i + 1 == nl ? w->head_w : nullptr;
        if (i == 0)
            NIR_PROPAGATE(conv2d_launch(nullptr, pd, pq, M, N, DL / 2, QL / 2, &w->l[0], NIR_ACT_RELU, hw, o[0], st, "nir_arcii_score (2-D layer)"));
        else
            NIR_PROPAGATE(conv2d_launch(o[i - 1], nullptr, nullptr, M, 1, hd[i - 1], hq[i - 1], &w->l[i], NIR_ACT_RELU, hw, o[i], st,
                                        "nir_arcii_score (2-D layer)"));
    }
    {
        const int n = hd[nl - 1] * hq[nl - 1] * (int)conv_ncb(w->l[nl - 1].F) * 2;
        ProfScope ps("arcii_finish_kernel", st);
        hipLaunchKernelGGL(arcii_finish_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, o[nl - 1], n, w->head_b, M, scores);
        NIR_CHECK_LAUNCH("nir_arcii_score (finish)");
    }
    return 0;
}
