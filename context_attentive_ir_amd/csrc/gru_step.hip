// One GRU decoder step (decoders/decoder.py:175-177, decoders/rnn_decoder.py:46-47: torch.nn.GRU, gate order r, z, n)
//     r = sigma(W_ir x + b_ir + W_hr h + b_hr),  z = sigma(W_iz x + b_iz + W_hz h + b_hz),
//     n = tanh(W_in x + b_in + r * (W_hn h + b_hn)),  h' = (1 - z) n + z h          (b_hn INSIDE the reset product)
// for the greedy decoders of Seq2seqGRU / ACGGRU (csrc/seq2seq.hip: s2s_decode) and, one step at a time, at the C ABI (nir_gru_step).
//
//   fast   gru_step16_kernel: ONE launch.  Input side from a per-token table gate_fold [V, 3H] = table W_ih^T + b_ih + (b_hr, b_hz, 0) gathered
//          by the previous step's token id (or from a [B, 3H] GEMM result when there is no table: then b_hr / b_hz are added here); recurrent
//          side W_hh h on the fp16 matrix cores over the two-term split (split2.hpp): W_hh pre-split in A-fragment order
//          (gru_step_whh_frag_kernel), h as the term pairs the previous step wrote.  H % 32 == 0, |w_hh| < 2^15.
//   plain  exact fp32, any H % 4 == 0: composed from launchers the library already has -- the gathered x W_ih^T + b_ih and h W_hh^T + b_hh
//          on the fp32-MFMA GEMM (launch_linear) and the cell of the training recurrence (nir_gru_cell_seq_fwd, csrc/gru_train.hip).  Three
//          launches; a fused fp32 kernel would repeat lstm_step_kernel for a path that only out-of-range weights, odd sizes and the
//          exact_f32 tunable take.
#include "decode_common.hpp"

namespace nir {

struct GruStep16Args {
    const float* gx;            // input side of the gates, row = [r | z | n] x H
    const int64_t* gxid;        // row b of gx is gx + gxid[b] * gxstride (folded table gathered by token id); NULL: row b
    int64_t gxstride;
    int64_t gxV;                // (gxid) ids outside [0, gxV) read row 1, <unk>
    const float* bhh;           // [3H]: b_hn always; b_hr, b_hz only when add_brz (the table holds them otherwise)
    int add_brz;
    const _Float16* whh_frag;   // gru_step_whh_frag_kernel's layout
    const float* hprev;         // [B,H]
    const _Float16* h16prev;    // [B][H/8][2 terms][8]
    float* hnext;
    _Float16* h16next;
    int B, H;
};

// A workgroup owns 16 hidden units: the r, z and n tiles (16 weight rows each) of the SAME units, so that after the product lane
// (i = batch column, g) holds units 4g .. 4g+3 of all three gates of its batch row and the cell needs no cross-lane traffic.  K = H is split
// over the four waves in 32-wide blocks (three v_mfma_f32_16x16x32_f16 each: w1 h1 -> acc, w1 h2' and w2' h1 -> acx), the four partial tiles
// are summed through LDS, and wave w finishes register w (unit 4g + w) of every batch tile.  NB batch tiles of 16 rows share one pass over the
// weights; further slabs of 16 NB rows go over blockIdx.z.  Rows past the batch are clamped on load and never stored.
template <int NB, int CK>
__global__ __launch_bounds__(256) void gru_step16_kernel(GruStep16Args p) {
    __shared__ float red[4][3][NB][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int H = p.H, KB = H >> 5, H8 = H >> 3;
    const int ug = blockIdx.x;                                 // H / 16 unit groups exactly (H % 32 == 0): nothing past the end
    const f16x8* wf = reinterpret_cast<const f16x8*>(p.whh_frag) + (size_t)ug * 3 * KB * 2 * 64 + lane;
    const int ud = 16 * ug + 4 * g + wave;                     // the unit this lane finishes
    const float bhn = p.bhh[2 * H + ud];
    const float bhr = p.add_brz ? p.bhh[ud] : 0.f, bhz = p.add_brz ? p.bhh[H + ud] : 0.f;
    for (int b0 = blockIdx.z * 16 * NB; b0 < p.B; b0 += gridDim.z * 16 * NB) {
        // the epilogue's operands first: their loads travel under the product
        float gxv[NB][3], hpv[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int bq = b0 + 16 * t + i;
            const int64_t brow = bq < p.B ? bq : p.B - 1;
            int64_t grow = brow;
            if (p.gxid) {
                grow = p.gxid[brow];
                grow = (grow >= 0 && grow < p.gxV) ? grow : 1;
            }
            const float* gr = p.gx + grow * p.gxstride + ud;
            gxv[t][0] = gr[0]; gxv[t][1] = gr[H]; gxv[t][2] = gr[2 * H];
            hpv[t] = p.hprev[brow * H + ud];
        }
        f32x4 acc[3][NB], acx[3][NB];
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                acc[q][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
                acx[q][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        const _Float16* hr[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int b = b0 + 16 * t + i;
            hr[t] = p.h16prev + ((int64_t)(b < p.B ? b : p.B - 1) * H8 + g) * 16;
        }
        for (int q0 = wave; q0 < KB; q0 += 4 * CK) {
            f16x8 w1[CK][3], w2[CK][3], h1[CK][NB], h2[CK][NB];
#pragma unroll
            for (int c = 0; c < CK; ++c) {
                const int kb = q0 + 4 * c;
                // past the end: block 0 again with zero weights (wave-uniform); the MFMAs below run unconditionally (see lstm_step16_kernel
                // for what a `continue` around them cost)
                const int kc = kb < KB ? kb : 0;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    w1[c][q] = wf[((size_t)q * KB + kc) * 2 * 64];
                    w2[c][q] = wf[((size_t)q * KB + kc) * 2 * 64 + 64];
                    if (kb >= KB) {
                        w1[c][q] = f16x8{};
                        w2[c][q] = f16x8{};
                    }
                }
#pragma unroll
                for (int t = 0; t < NB; ++t) {
                    h1[c][t] = *reinterpret_cast<const f16x8*>(hr[t] + (int64_t)kc * 64);
                    h2[c][t] = *reinterpret_cast<const f16x8*>(hr[t] + (int64_t)kc * 64 + 8);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < CK; ++c)
#pragma unroll
                for (int q = 0; q < 3; ++q)
#pragma unroll
                    for (int t = 0; t < NB; ++t) {
                        acc[q][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[c][q], h1[c][t], acc[q][t], 0, 0, 0);
                        acx[q][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[c][q], h2[c][t], acx[q][t], 0, 0, 0);
                        acx[q][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2[c][q], h1[c][t], acx[q][t], 0, 0, 0);
                    }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int t = 0; t < NB; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[wave][q][t][r * 64 + lane] = split2_combine(acc[q][t][r], acx[q][t][r]);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            float s[3];
#pragma unroll
            for (int q = 0; q < 3; ++q)
                s[q] = (red[0][q][t][wave * 64 + lane] + red[1][q][t][wave * 64 + lane]) + (red[2][q][t][wave * 64 + lane] + red[3][q][t][wave * 64 + lane]);
            const int b = b0 + 16 * t + i;
            const float rg = fast_sigmoid((gxv[t][0] + bhr) + s[0]);
            const float zg = fast_sigmoid((gxv[t][1] + bhz) + s[1]);
            const float ng = fast_tanh(gxv[t][2] + rg * (s[2] + bhn));
            float hn = (1.f - zg) * ng + zg * hpv[t];
            // pin hn as the fp32 value that is stored: without it the compiler folds the fp16 conversion below into the blend (v_fma_mixlo_f16,
            // ONE rounding of the exact sum), and at an fp16 tie h1 is then not the rounding of the stored h_next
            asm volatile("" : "+v"(hn));
            if (b < p.B) {
                p.hnext[(int64_t)b * H + ud] = hn;
                const _Float16 a = split2_hi1_rne(hn);         // the next step's B operand: the two fp16 terms
                _Float16* d = p.h16next + ((int64_t)b * H8 + (ud >> 3)) * 16 + (ud & 7);
                d[0] = a;
                d[8] = split2_lo1(hn, a);
            }
        }
        __syncthreads();
    }
}

// W_hh [3H, H] -> [H/16 unit groups][3 gates][H/32 k-blocks][2 terms][64 lanes][8]: lane (i, g) of (ug, gate, kb) holds k = 32 kb + 8 g .. + 7 of
// weight row gate * H + 16 ug + i -- the A fragment of gru_step16_kernel.  err |= 2 when a weight is outside the split's range (|w| >= 2^15 or NaN).
__global__ __launch_bounds__(64) void gru_step_whh_frag_kernel(const float* __restrict__ whh, int H, _Float16* __restrict__ out, int* __restrict__ err) {
    const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
    const int ug = blockIdx.x, kb = blockIdx.y, gate = blockIdx.z, KB = H >> 5;
    const float* wr = whh + ((int64_t)gate * H + 16 * ug + i) * H + 32 * kb + 8 * g;
    _Float16* o = out + ((((int64_t)ug * 3 + gate) * KB + kb) * 2 * 64 + lane) * 8;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float w = wr[j];
        const _Float16 a = split2_hi1_rne(w);
        o[j] = a;
        o[64 * 8 + j] = split2_lo1(w, a);
        bad |= !(fabsf(w) < 32768.0f);
    }
    if (bad && err) atomicOr(err, 2);
}

// ids outside [0, V) -> 1 (<unk>), like the arg-max kernels' next tokens
__global__ void gru_step_ids_kernel(const int64_t* __restrict__ ids, int64_t V, int64_t n, int64_t* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) {
        const int64_t v = ids[e];
        out[e] = (v >= 0 && v < V) ? v : 1;
    }
}

bool gru_step_fast(const GruStepArgs& a) {
    return a.whh_frag && a.h16prev && a.h16next && a.H % 32 == 0 && !tun(g_tun.exact_f32);
}

size_t gru_step_scratch_floats(int64_t B, int H) { return (size_t)10 * B * H; }

int launch_gru_step(const GruStepArgs& a, hipStream_t st) {
    NIR_REQUIRE(a.H > 0 && a.H % 4 == 0 && a.B >= 0 && a.B < 0x7FFFFFFFLL, "gru_step: H must be a positive multiple of 4");
    NIR_REQUIRE(a.tok && a.bhh && a.hprev && a.hnext, "gru_step: null pointer");
    if (a.B == 0) return 0;
    const int H = a.H;
    const int64_t B = a.B;
    const bool fast = gru_step_fast(a);
    float* gx = a.scratch;                                    // [B,3H]; then gh [B,3H] and act [B,4H] of the plain form
    if (!(fast && a.gate_fold)) {                             // x W_ih^T + b_ih, rows gathered by token id
        NIR_REQUIRE(a.table && a.wih && a.bih && a.E > 0 && a.E % 4 == 0 && gx, "gru_step: no gate table and no (table, w_ih, b_ih, scratch)");
        NIR_PROPAGATE(launch_linear(nullptr, 0, a.tok, a.table, a.E, 1, 1, a.wih, a.E, a.bih, nullptr, gx, 3 * H, B, 3 * H, a.E, NIR_ACT_NONE, st));
    }
    if (fast) {
        GruStep16Args k;
        k.gx = a.gate_fold ? a.gate_fold : gx;
        k.gxid = a.gate_fold ? a.tok : nullptr;
        k.gxstride = (int64_t)3 * H; k.gxV = a.V;
        k.bhh = a.bhh; k.add_brz = a.gate_fold ? 0 : 1;
        k.whh_frag = reinterpret_cast<const _Float16*>(a.whh_frag);
        k.hprev = a.hprev; k.h16prev = a.h16prev; k.hnext = a.hnext; k.h16next = a.h16next;
        k.B = (int)B; k.H = H;
        ProfScope ps("gru_step16_kernel", st);
        // batch tiles per workgroup as in launch_lstm_step: the step is a latency chain, more and smaller workgroups win
        const int NBv = B > 32 ? 4 : (B > 16 ? 2 : 1);
        const dim3 grid((unsigned)(H / 16), 1, (unsigned)((B + 16 * NBv - 1) / (16 * NBv)));
        if (NBv == 4) hipLaunchKernelGGL((gru_step16_kernel<4, 2>), grid, dim3(256), 0, st, k);
        else if (NBv == 2) hipLaunchKernelGGL((gru_step16_kernel<2, 4>), grid, dim3(256), 0, st, k);
        else hipLaunchKernelGGL((gru_step16_kernel<1, 4>), grid, dim3(256), 0, st, k);
        NIR_CHECK_LAUNCH("gru_step16_kernel");
        return 0;
    }
    NIR_REQUIRE(a.whh, "gru_step: null w_hh");
    float* gh = gx + (size_t)3 * B * H;
    float* act = gh + (size_t)3 * B * H;
    NIR_PROPAGATE(launch_linear(a.hprev, H, nullptr, nullptr, 0, 0, 0, a.whh, H, a.bhh, nullptr, gh, 3 * H, B, 3 * H, H, NIR_ACT_NONE, st));
    NIR_PROPAGATE(nir_gru_cell_seq_fwd(gx, 3 * H, gh, a.bhh, a.hprev, H, act, 4 * H, a.hnext, H, B, H, (nir_stream_t)st));
    if (a.h16next && H % 8 == 0) NIR_PROPAGATE(launch_h16_pack(a.hnext, B * H, a.h16next, st));
    return 0;
}

}  // namespace nir

extern "C" size_t nir_gru_step_whh_frag_bytes(int H) { return (H > 0 && H % 32 == 0) ? (size_t)3 * H * H * 2 * sizeof(_Float16) : 0; }

extern "C" int nir_gru_step_pack_whh_frag(const float* w_hh, int H, void* frag, int* err_flag, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(w_hh && frag && H > 0 && H % 32 == 0, "gru_step_pack_whh_frag: H must be a positive multiple of 32");
    hipLaunchKernelGGL(gru_step_whh_frag_kernel, dim3((unsigned)(H / 16), (unsigned)(H / 32), 3), dim3(64), 0, (hipStream_t)stream, w_hh, H, (_Float16*)frag,
                       err_flag);
    NIR_CHECK_LAUNCH("gru_step_whh_frag_kernel");
    return 0;
}

// workspace of nir_gru_step: clamped ids, the plain form's gates, and the fp16 term pairs the caller did not bring
namespace nir {
struct GruStepPlan {
    int64_t* ids;
    float* scratch;
    _Float16 *h16p, *h16n;
    size_t bytes;
};
static GruStepPlan gru_step_plan(void* ws, size_t cap, int64_t B, int H) {
    Workspace a(ws, cap);
    GruStepPlan p;
    p.ids = a.take<int64_t>((size_t)B);
    p.scratch = a.take<float>(gru_step_scratch_floats(B, H));
    p.h16p = a.take<_Float16>((size_t)2 * B * H);
    p.h16n = a.take<_Float16>((size_t)2 * B * H);
    p.bytes = align_up(a.off, 256);
    return p;
}
}  // namespace nir

extern "C" size_t nir_gru_step_workspace_bytes(int64_t B, int H) {
    if (B < 0 || H <= 0 || H % 4) return 0;
    return nir::gru_step_plan(nullptr, 0, B, H).bytes;
}

extern "C" int nir_gru_step(const int64_t* ids, int64_t B, const float* table, int64_t V, int E, const float* w_ih, const float* b_ih,
                            const float* gate_fold, const float* w_hh, const float* b_hh, const void* whh_frag, int H, const float* h_prev,
                            const void* h16_prev, float* h_next, void* h16_next, void* workspace, size_t workspace_bytes, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(ids && w_hh && b_hh && h_prev && h_next, "gru_step: null pointer");
    NIR_REQUIRE(B >= 0 && B < 0x7FFFFFFFLL && H > 0 && H % 4 == 0 && V > 1, "gru_step: bad dims (H a positive multiple of 4, V > 1)");
    NIR_REQUIRE(gate_fold || (table && w_ih && b_ih && E > 0 && E % 4 == 0), "gru_step: gate_fold, or table / w_ih / b_ih with E a positive multiple of 4");
    GruStepPlan p = gru_step_plan(workspace, workspace_bytes, B, H);
    if (!workspace || p.bytes > workspace_bytes) {
        set_error("gru_step: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
        return NIR_ERR_WORKSPACE;
    }
    if (B == 0) return 0;
    hipLaunchKernelGGL(gru_step_ids_kernel, g1(B), dim3(256), 0, st, ids, V, B, p.ids);
    NIR_CHECK_LAUNCH("gru_step_ids_kernel");
    GruStepArgs a;
    a.tok = p.ids; a.V = V; a.gate_fold = gate_fold;
    a.table = table; a.E = E; a.wih = w_ih; a.bih = b_ih;
    a.whh = w_hh; a.bhh = b_hh; a.whh_frag = H % 32 == 0 ? whh_frag : nullptr;
    a.hprev = h_prev; a.hnext = h_next;
    a.h16prev = reinterpret_cast<const _Float16*>(h16_prev);
    a.h16next = reinterpret_cast<_Float16*>(h16_next);
    a.scratch = p.scratch; a.B = B; a.H = H;
    if (a.whh_frag && !tun(g_tun.exact_f32)) {               // the fast form: bring the term pairs the caller left out
        if (!a.h16prev) {
            NIR_PROPAGATE(launch_h16_pack(h_prev, B * H, p.h16p, st));
            a.h16prev = p.h16p;
        }
        if (!a.h16next) a.h16next = p.h16n;
    }
    return launch_gru_step(a, st);
}
