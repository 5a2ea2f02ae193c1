// ACG -- the Seq2seq recommender with a copy generator (neuroir/recommender/seq2seq.py with copy_attn; modules/copy_generator.py:57-135;
// utils/copy_utils.py:5-39).  The decode is Seq2seq's (csrc/seq2seq.hip: s2s_decode) up to the attentional output o [B, H]; what changes is
// the choice of the next token.  With l = W_g o + b_g (l[PAD] := -1e-20), s = softmax(l), z = sigmoid(w_c . o + b_c) and the copy attention a:
//   P[v]      = (1 - z) s[v]                                  v < VT
//   P[VT + c] = z sum_{j < len, map[j] = c} a[j]              c < CV: the row's own dynamic dictionary
//   collapse:   every slot c >= 2 whose word has a target id t: P[t] += P[VT + c], P[VT + c] = 1e-10
//   pred = argmax P (first index on ties), an EXTENDED id in [0, VT + CV); the token fed back is tgt2src[pred] or ext2src[b, pred - VT].
// The reference writes the [B, VT + CV] matrix every step and collapses row by row on the host.  Here a step is two launches:
//   s2s_gen_argmax_kernel<NBT, true> (s2s_gen.hpp)   per wave and row one (max, index, sum exp(l - max)) partial; the logits are never written
//       (plain form: fp32 GEMM into workspace logits + acg_row_stats_kernel, one partial per row)
//   acg_select_kernel                                 merges the partials, forms z and the copy mass of every slot, and compares the only
//       entries of P that can win: the vocabulary's own winner, the un-collapsed slots, and every collapsed target t with its copy mass added
//       (l[t] from one fp32 dot of o with generator row t).
// The rows of the teacher-forced loss (CopyGeneratorCriterion) are at the bottom.  fp32 throughout, vector stores only, no float atomics.
#include <algorithm>
#include "s2s_gen.hpp"

namespace nir {

__device__ __forceinline__ float acg_block_reduce(float v, float* red, bool is_max) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = is_max ? wave_max(v) : wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < 4; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

// ---- plain form: the statistics of a row of workspace logits, in the partial format of the fused kernel (one partial per row) ---------
__global__ __launch_bounds__(256) void acg_row_stats_kernel(const float* __restrict__ logits, int64_t VT, float* __restrict__ pval, int* __restrict__ pidx,
                                                            float* __restrict__ psum) {
    __shared__ float red[4];
    __shared__ int redi[4];
    const float* zr = logits + (int64_t)blockIdx.x * VT;
    float m = -INFINITY;
    for (int64_t v = threadIdx.x; v < VT; v += 256) m = fmaxf(m, v == 0 ? ACG_PAD_LOGIT : zr[v]);
    m = acg_block_reduce(m, red, true);
    int first = 0x7FFFFFFF;                                   // the first index that holds the maximum
    float s = 0.f;
    for (int64_t v = threadIdx.x; v < VT; v += 256) {
        const float y = v == 0 ? ACG_PAD_LOGIT : zr[v];
        if (y == m && (int)v < first) first = (int)v;
        s += __expf(y - m);
    }
    s = acg_block_reduce(s, red, false);
    for (int sh = 32; sh >= 1; sh >>= 1) first = min(first, __shfl_xor(first, sh));
    if ((threadIdx.x & 63) == 0) redi[threadIdx.x >> 6] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        pval[blockIdx.x] = m;
        pidx[blockIdx.x] = min(min(redi[0], redi[1]), min(redi[2], redi[3]));
        psum[blockIdx.x] = s;
    }
}

// ---- the choice of the next token: one wave per decode row -------------------------------------------------------------------------------
// (value, extended id) candidates are compared with `>` and the lower id on equal values, the order torch.max reads the reference's row in.
__device__ __forceinline__ void acg_better(float v, int64_t id, float& bv, int64_t& bid) {
    if (v > bv || (v == bv && id < bid)) { bv = v; bid = id; }
}

__global__ __launch_bounds__(256) void acg_select_kernel(const float* __restrict__ o, int K, const float* __restrict__ gen_w, const float* __restrict__ gen_b,
                                                         int64_t VT, const float* __restrict__ pval, const int* __restrict__ pidx,
                                                         const float* __restrict__ psum, int nparts, const float* __restrict__ copy_w,
                                                         const float* __restrict__ copy_b, const float* __restrict__ attn, int64_t attn_stride,
                                                         const int64_t* __restrict__ lens, int QL, const int64_t* __restrict__ map,
                                                         const int64_t* __restrict__ e2t, const int64_t* __restrict__ e2s, int CV,
                                                         const int64_t* __restrict__ lut, int64_t Vsrc, int64_t Bd, int64_t* __restrict__ pred,
                                                         int64_t pstride, int64_t* __restrict__ tgt, float* __restrict__ stat_max,
                                                         float* __restrict__ stat_lse, int64_t* __restrict__ stat_idx) {
    extern __shared__ float acg_sm[];                          // per wave: mass [CV] floats, tl [CV] ints
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= Bd) return;                                       // wave-uniform; no workgroup barrier below
    float* mass = acg_sm + (size_t)wave * 2 * CV;
    int* tl = reinterpret_cast<int*>(mass + CV);
    // 1. the generator's statistics: m = max_v l[v] at idx (first index), Z = sum_v exp(l[v] - m)
    float m = -INFINITY, Z = 0.f;
    int idx = 0x7FFFFFFF;
    auto merge = [&](float pv, int pi, float ps) {
        const float M = fmaxf(m, pv);
        if (M > -INFINITY) Z = Z * expf(m - M) + ps * expf(pv - M);
        if (pv > m || (pv == m && pi < idx)) idx = pi;
        m = M;
    };
    for (int p = lane; p < nparts; p += 64) merge(pval[(int64_t)p * Bd + b], pidx[(int64_t)p * Bd + b], psum[(int64_t)p * Bd + b]);
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const float ov = __shfl_xor(m, sh), os = __shfl_xor(Z, sh);
        const int oi = __shfl_xor(idx, sh);
        merge(ov, oi, os);
    }
    m = __shfl(m, 0); Z = __shfl(Z, 0); idx = __shfl(idx, 0);  // one lane's rounding for the whole wave
    if (idx < 0 || idx >= VT) idx = 0;
    if (lane == 0) {
        if (stat_max) stat_max[b] = m;
        if (stat_lse) stat_lse[b] = m + logf(Z);
        if (stat_idx) stat_idx[b] = idx;
    }
    // 2. the copy switch z = sigmoid(w_c . o + b_c); 1 - z is formed as sigmoid(-x): it keeps its precision where z rounds to 1
    const float* ob = o + b * K;
    float x = 0.f;
    for (int k = 4 * lane; k < K; k += 256) {
        const float4 a = *reinterpret_cast<const float4*>(ob + k), w = *reinterpret_cast<const float4*>(copy_w + k);
        x += (a.x * w.x + a.y * w.y) + (a.z * w.z + a.w * w.w);
    }
    x = wave_sum(x) + copy_b[0];
    const float z = 1.0f / (1.0f + expf(-x)), omz = 1.0f / (1.0f + expf(x));
    // 3. the copy mass of every dictionary slot (a gather per slot, in ascending j like the reference's bmm: no atomics; map entries at
    //    j >= len are never read) and the slot's target id, -1 where the slot is not collapsed (slots 0 and 1 never are)
    int len = (int)lens[b];
    len = len < 0 ? 0 : (len > QL ? QL : len);
    const int64_t* mb = map + b * QL;
    const float* ab = attn + b * attn_stride;
    for (int c = lane; c < CV; c += 64) {
        float acc = 0.f;
        for (int j = 0; j < len; ++j)
            if (mb[j] == c) acc += z * ab[j];
        mass[c] = acc;
        const int64_t t = e2t[b * CV + c];
        tl[c] = (c >= 2 && t >= 0 && t < VT) ? (int)t : -1;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // 4. the candidates.  A collapsed slot itself holds 1e-10 in the reference; the largest of the VT + CV entries, which sum to 1, is at least
    //    1 / (VT + CV) > 1e-10 for any dictionary below 10^10 entries, so such a slot never wins and needs no candidate.
    float bv = omz / Z;                                        // the vocabulary's own winner: (1 - z) exp(m - m) / Z at idx.  If idx is a collapsed
    int64_t bid = idx;                                         // target, its candidate below has the same id and at least this value
    for (int c = lane; c < CV; c += 64)
        if (tl[c] < 0) acg_better(mass[c], VT + c, bv, bid);
    for (int c = 2; c < CV; ++c) {                             // wave-uniform: every slot that is the FIRST of its target id
        const int t = tl[c];
        if (t < 0) continue;
        int dup = 0;
        float cp = 0.f;
        for (int c2 = lane; c2 < CV; c2 += 64)
            if (tl[c2] == t) {
                if (c2 < c) dup = 1;
                else cp += mass[c2];
            }
        if (__any(dup)) continue;
        cp = wave_sum(cp);                                     // index_add_ accumulates the slots that share t
        float lt = ACG_PAD_LOGIT;
        if (t != 0) {
            const float* wr = gen_w + (int64_t)t * K;
            float d = 0.f;
            for (int k = 4 * lane; k < K; k += 256) {
                const float4 a = *reinterpret_cast<const float4*>(ob + k), w = *reinterpret_cast<const float4*>(wr + k);
                d += (a.x * w.x + a.y * w.y) + (a.z * w.z + a.w * w.w);
            }
            lt = wave_sum(d) + (gen_b ? gen_b[t] : 0.f);
        }
        acg_better(omz * expf(lt - m) / Z + cp, (int64_t)t, bv, bid);
    }
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const float ov = __shfl_xor(bv, sh);
        const int64_t oi = __shfl_xor(bid, sh);
        acg_better(ov, oi, bv, bid);
    }
    if (lane == 0) {
        int64_t tok = bid < VT ? (lut ? lut[bid] : bid) : e2s[b * CV + (bid - VT)];
        if (tok < 0 || tok >= Vsrc) tok = 1;                   // <unk>, as launch_argmax_map does
        pred[b * pstride] = bid;
        tgt[b] = tok;
    }
}

static int launch_acg_gen_select_stats(const float* o, int64_t B, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                                       float* logits, float* pval, int* pidx, float* psum, const float* copy_w, const float* copy_b, const float* attn,
                                       int64_t attn_stride, const int64_t* lens, int QL, const int64_t* src_map_idx, const int64_t* ext2tgt,
                                       const int64_t* ext2src, int CV, const int64_t* tgt2src, int64_t V, int64_t* pred, int64_t pstride, int64_t* tgt,
                                       float* stat_max, float* stat_lse, int64_t* stat_idx, hipStream_t st) {
    int nparts = 1;
    if (gen_frag) {
        NIR_PROPAGATE(launch_gen_argmax_partials<true>("s2s_gen_stats_kernel", o, gen_frag, gen_b, VT, B, K, pval, pidx, psum, &nparts, st));
    } else {
        NIR_PROPAGATE(launch_linear(o, K, nullptr, nullptr, 0, 0, 0, gen_w, K, gen_b, nullptr, logits, VT, B, (int)VT, K, NIR_ACT_NONE, st));
        {
            ProfScope ps("acg_row_stats_kernel", st);
            hipLaunchKernelGGL(acg_row_stats_kernel, dim3((unsigned)B), dim3(256), 0, st, logits, VT, pval, pidx, psum);
        }
        NIR_CHECK_LAUNCH("acg_row_stats_kernel");
    }
    {
        ProfScope ps("acg_select_kernel", st);
        hipLaunchKernelGGL(acg_select_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), (size_t)4 * 2 * CV * sizeof(float), st, o, K, gen_w, gen_b, VT, pval,
                           pidx, psum, nparts, copy_w, copy_b, attn, attn_stride, lens, QL, src_map_idx, ext2tgt, ext2src, CV, tgt2src, V, B, pred, pstride,
                           tgt, stat_max, stat_lse, stat_idx);
    }
    NIR_CHECK_LAUNCH("acg_select_kernel");
    return 0;
}

int launch_acg_gen_select(const float* o, int64_t B, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT, float* logits,
                          float* pval, int* pidx, float* psum, const float* copy_w, const float* copy_b, const float* attn, int64_t attn_stride,
                          const int64_t* lens, int QL, const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src, int CV,
                          const int64_t* tgt2src, int64_t V, int64_t* pred, int64_t pstride, int64_t* tgt, hipStream_t st) {
    return launch_acg_gen_select_stats(o, B, K, gen_w, gen_b, gen_frag, VT, logits, pval, pidx, psum, copy_w, copy_b, attn, attn_stride, lens, QL,
                                       src_map_idx, ext2tgt, ext2src, CV, tgt2src, V, pred, pstride, tgt, nullptr, nullptr, nullptr, st);
}

// ---- the rows of the teacher-forced loss (CopyGeneratorCriterion, copy_generator.py:99-135) ---------------------------------------------
// Per row r with logits l [V] (l[PAD] := -1e-20), switch logit x, copy mass c = sum_{j: map[j] = al} a[j], target t and alignment al:
//   z = sigmoid(x), s_t = softmax(l)[t],  A = [al != UNK] z c,  w = [t != UNK] + [al = UNK][t = UNK]  (force_copy: w = [al = UNK])
//   out = A + 1e-20 + w (1 - z) s_t,  loss = -log(out)        (the PAD mask of seq2seq.py:101 is the caller's)
struct AcgLossRow { float z, omz, st, w, anu, out; };
__device__ __forceinline__ AcgLossRow acg_loss_row(const float* zr, int V, float lse, float x, float mass, int64_t t, int64_t al, int force_copy) {
    AcgLossRow q;
    q.z = 1.0f / (1.0f + expf(-x));
    q.omz = 1.0f / (1.0f + expf(x));
    const bool ok = t >= 0 && t < V;
    q.st = ok ? expf((t == 0 ? ACG_PAD_LOGIT : zr[t]) - lse) : 0.f;
    q.anu = al != 1 ? 1.f : 0.f;
    q.w = force_copy ? (al == 1 ? 1.f : 0.f) : ((t != 1 ? 1.f : 0.f) + ((al == 1 && t == 1) ? 1.f : 0.f));
    q.out = q.anu * q.z * mass + 1e-20f + q.w * q.omz * q.st;
    return q;
}

__global__ __launch_bounds__(256) void acg_copy_loss_fwd_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ sw,
                                                                const float* __restrict__ mass, const int64_t* __restrict__ target,
                                                                const int64_t* __restrict__ align, int force_copy, int V, float* __restrict__ loss,
                                                                float* __restrict__ lse, int* err) {
    __shared__ float red[4];
    const int64_t r = blockIdx.x;
    const float* zr = logits + r * ld;
    float m = -INFINITY;
    for (int v = threadIdx.x; v < V; v += 256) m = fmaxf(m, v == 0 ? ACG_PAD_LOGIT : zr[v]);
    m = acg_block_reduce(m, red, true);
    float s = 0.f;
    for (int v = threadIdx.x; v < V; v += 256) s += expf((v == 0 ? ACG_PAD_LOGIT : zr[v]) - m);
    s = acg_block_reduce(s, red, false);
    if (threadIdx.x == 0) {
        const float l = m + logf(s);
        const int64_t t = target[r];
        if (!(t >= 0 && t < V) && err) atomicOr(err, 1);
        const AcgLossRow q = acg_loss_row(zr, V, l, sw[r], mass[r], t, align[r], force_copy);
        lse[r] = l;
        loss[r] = -logf(q.out);
    }
}

// dlogits[v] = -g w (1 - z) s_t ([v = t] - s_v) / out (0 in the PAD column: its logit is a constant), d switch logit, d mass: one pass
__global__ __launch_bounds__(256) void acg_copy_loss_bwd_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ sw,
                                                                const float* __restrict__ mass, const int64_t* __restrict__ target,
                                                                const int64_t* __restrict__ align, int force_copy, const float* __restrict__ lse,
                                                                const float* __restrict__ gloss, int V, float* __restrict__ dz, float* __restrict__ dsw,
                                                                float* __restrict__ dmass) {
    const int64_t r = blockIdx.y;
    const float* zr = logits + r * ld;
    const float l = lse[r], g = gloss[r];
    const int64_t t = target[r];
    const AcgLossRow q = acg_loss_row(zr, V, l, sw[r], mass[r], t, align[r], force_copy);
    const float go = -g / q.out;
    const float coef = go * (q.w * q.omz * q.st);
    float* dr = dz + r * (int64_t)V;
    const int v0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    for (int v = v0; v < min(V, v0 + 4); ++v)
        dr[v] = v == 0 ? 0.f : coef * ((v == t ? 1.f : 0.f) - expf(zr[v] - l));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        dsw[r] = go * (q.anu * mass[r] - q.w * q.st) * q.z * q.omz;
        dmass[r] = go * q.anu * q.z;
    }
}

static size_t acg_gen_select_bytes(int64_t rows, int64_t VT, bool fused) {
    const size_t parts = fused ? (size_t)S2S_MAX_WGS * 4 * rows : (size_t)rows;
    return (fused ? 0 : align_up((size_t)rows * VT * sizeof(float), 256)) + 3 * align_up(parts * 4, 256) + 256;
}

}  // namespace nir

extern "C" size_t nir_acg_gen_select_workspace_bytes(int64_t rows, int K, int64_t VT, int fused) {
    if (rows <= 0 || K <= 0 || VT <= 0) return 0;
    return nir::acg_gen_select_bytes(rows, VT, fused != 0);
}

extern "C" int nir_acg_gen_select(const float* o, int64_t rows, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                                  const float* copy_w, const float* copy_b, const float* copy_attn, int64_t attn_stride, const int64_t* source_len, int QL,
                                  const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src, int CV, const int64_t* tgt2src, int64_t V,
                                  void* workspace, size_t workspace_bytes, int64_t* predictions, int64_t pred_stride, int64_t* next_tokens,
                                  float* stat_max, float* stat_lse, int64_t* stat_idx, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(o && gen_w && copy_w && copy_b && copy_attn && source_len && src_map_idx && ext2tgt && ext2src && predictions && next_tokens && workspace,
                "acg_gen_select: null pointer");
    NIR_REQUIRE(rows >= 0 && K > 0 && K % 4 == 0 && VT > 0 && VT < 0x7FFFFFF0LL && V > 0 && pred_stride >= 1 && attn_stride >= QL, "acg_gen_select: bad dims");
    NIR_REQUIRE(acg_dims_ok(QL, CV), "acg_gen_select: QL outside [1, 4096] or CV outside [2, %d]", ACG_MAX_CV);
    const bool fused = s2s_gen_fused(gen_frag, K, VT);
    if (workspace_bytes < acg_gen_select_bytes(rows, VT, fused)) {
        set_error("acg_gen_select: workspace too small");
        return NIR_ERR_WORKSPACE;
    }
    if (rows == 0) return 0;
    Workspace a(workspace, workspace_bytes);
    const size_t parts = fused ? (size_t)S2S_MAX_WGS * 4 * rows : (size_t)rows;
    float* logits = a.take<float>(fused ? 0 : (size_t)rows * VT);
    float* pval = a.take<float>(parts);
    int* pidx = a.take<int>(parts);
    float* psum = a.take<float>(parts);
    return launch_acg_gen_select_stats(o, rows, K, gen_w, gen_b, fused ? gen_frag : nullptr, VT, logits, pval, pidx, psum, copy_w, copy_b, copy_attn,
                                       attn_stride, source_len, QL, src_map_idx, ext2tgt, ext2src, CV, tgt2src, V, predictions, pred_stride, next_tokens,
                                       stat_max, stat_lse, stat_idx, st);
}

extern "C" size_t nir_acg_decode_workspace_bytes(int64_t B, int QL, int CV, const nir_seq2seq_decoder_weights* w, const nir_acg_copy_weights* cw) {
    if (!cw || !nir::acg_dims_ok(QL, CV)) return 0;
    nir::AcgDecode g{cw, nullptr, nullptr, nullptr, CV};
    return nir::s2s_decode_workspace_bytes(B, QL, w, &g, nir::S2S_CELL_LSTM);
}

extern "C" int nir_acg_decode_greedy(const float* dec_h, const float* dec_c, const float* memory_bank, const int64_t* source_len, int64_t B, int QL,
                                     const float* table, int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len,
                                     const nir_seq2seq_decoder_weights* w, const nir_acg_copy_weights* cw, const int64_t* src_map_idx,
                                     const int64_t* ext2tgt, const int64_t* ext2src, int CV, void* workspace, size_t workspace_bytes,
                                     int64_t* predictions, float* attentions, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(cw, "acg_decode: null copy weights");
    AcgDecode g{cw, src_map_idx, ext2tgt, ext2src, CV};
    return s2s_decode(dec_h, dec_c, memory_bank, source_len, B, QL, table, V, E, tgt2src, bos, max_len, w, workspace, workspace_bytes, predictions, attentions,
                      &g, S2S_CELL_LSTM, (hipStream_t)stream);
}

// The same decode with a GRU decoder (nir_seq2seq_gru_decode_greedy's step in front of the copy generator)
extern "C" size_t nir_acg_gru_decode_workspace_bytes(int64_t B, int QL, int CV, const nir_seq2seq_decoder_weights* w, const nir_acg_copy_weights* cw) {
    if (!cw || !nir::acg_dims_ok(QL, CV)) return 0;
    nir::AcgDecode g{cw, nullptr, nullptr, nullptr, CV};
    return nir::s2s_decode_workspace_bytes(B, QL, w, &g, nir::S2S_CELL_GRU);
}

extern "C" int nir_acg_gru_decode_greedy(const float* dec_h, const float* memory_bank, const int64_t* source_len, int64_t B, int QL, const float* table,
                                         int64_t V, int E, const int64_t* tgt2src, int64_t bos, int max_len, const nir_seq2seq_decoder_weights* w,
                                         const nir_acg_copy_weights* cw, const int64_t* src_map_idx, const int64_t* ext2tgt, const int64_t* ext2src,
                                         int CV, void* workspace, size_t workspace_bytes, int64_t* predictions, float* attentions,
                                         nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(cw, "acg_decode: null copy weights");
    AcgDecode g{cw, src_map_idx, ext2tgt, ext2src, CV};
    return s2s_decode(dec_h, nullptr, memory_bank, source_len, B, QL, table, V, E, tgt2src, bos, max_len, w, workspace, workspace_bytes, predictions,
                      attentions, &g, S2S_CELL_GRU, (hipStream_t)stream);
}

extern "C" int nir_acg_copy_loss_fwd(const float* logits, int64_t ld, const float* switch_logit, const float* copy_mass, const int64_t* target,
                                     const int64_t* align, int force_copy, int64_t R, int V, float* loss, float* lse, int* err_flag,
                                     nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(logits && switch_logit && copy_mass && target && align && loss && lse && R >= 0 && V > 0 && ld >= V, "acg_copy_loss_fwd: bad args");
    if (R == 0) return 0;
    hipLaunchKernelGGL(acg_copy_loss_fwd_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, logits, ld, switch_logit, copy_mass, target, align,
                       force_copy, V, loss, lse, err_flag);
    NIR_CHECK_LAUNCH("acg_copy_loss_fwd_kernel");
    return 0;
}

extern "C" int nir_acg_copy_loss_bwd(const float* logits, int64_t ld, const float* switch_logit, const float* copy_mass, const int64_t* target,
                                     const int64_t* align, int force_copy, const float* lse, const float* grad_loss, int64_t R, int V, float* dlogits,
                                     float* dswitch, float* dmass, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(logits && switch_logit && copy_mass && target && align && lse && grad_loss && dlogits && dswitch && dmass && R >= 0 && R < 65536 && V > 0 &&
                    ld >= V,
                "acg_copy_loss_bwd: bad args (rows < 65536)");
    if (R == 0) return 0;
    hipLaunchKernelGGL(acg_copy_loss_bwd_kernel, dim3((unsigned)((V + 1023) / 1024), (unsigned)R), dim3(256), 0, (hipStream_t)stream, logits, ld, switch_logit,
                       copy_mass, target, align, force_copy, lse, grad_loss, V, dlogits, dswitch, dmass);
    NIR_CHECK_LAUNCH("acg_copy_loss_bwd_kernel");
    return 0;
}
