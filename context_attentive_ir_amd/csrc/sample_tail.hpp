// The sampling tail as the decodes see it (csrc/sample.hip, csrc/session_sample.hip; DESIGN.md sections 28 and 29): the key of the noise, where a
// row's choice goes, the argument checks and the launchers.  The kernels live in csrc/sample.hip; these are their host-side launchers.
#pragma once
#include <cmath>
#include "common.hpp"

namespace nir {

constexpr int SAMPLE_NONE = 0x7FFFFFFF;               // the index of "no candidate yet"

// ---- the noise: one function for every form ------------------------------------------------------------------------------------------------
struct SampleKey {
    uint32_t k0, k1, step;                            // the seed's halves; the step t
    uint32_t nsrc;                                    // decode row r draws as (source row r % nsrc, sample r / nsrc)
};
static inline SampleKey sample_key(uint64_t seed, int64_t step, int64_t nsrc) {
    return SampleKey{(uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)nsrc};
}

// ---- where a row's choice goes ------------------------------------------------------------------------------------------------------------------
// Kernel-level entries (fin == NULL): token / logp / lse [rows], no freeze, no feedback.  Decode (fin given): the freeze rule on the row's state
// fin / cum / len [rows] (row order r = n nsrc + b), column `step` of predictions and token_logprobs [nsrc, N, max_len], and the id the next
// step reads, through lut (tgt2src), <unk> (1) outside [0, Vsrc).
struct SampleOut {
    int32_t* token;
    float *logp, *lse;
    int* fin;
    float* cum;
    int64_t* len;
    int64_t* pred;
    float* tlp;
    int64_t* next_ids;
    const int64_t* lut;
    int64_t Vsrc, VT, nsrc;
    int N, step, max_len;
    // the copy generator's sampler: ids in [VT, VT + CV) are dictionary slots of source row `row % nsrc`, fed back through
    // e2s [nsrc, CV]; CV = 0 everywhere else
    const int64_t* e2s = nullptr;
    int CV = 0;
};

static inline bool sample_tau_ok(float inv_tau) { return std::isfinite(inv_tau) && inv_tau > 0.f; }
static inline bool sample_key_ok(int64_t step, int64_t nsrc, int64_t rows) { return step >= 0 && step <= 0xFFFFFFFFLL && nsrc >= 1 && nsrc < 0x7FFFFFFFLL && rows >= 0 && rows < 0x7FFFFFFFLL; }
static inline bool sample_dims_ok(int N, int top_k, int64_t VT) { return N >= 1 && top_k >= 0 && top_k <= NIR_BEAM_MAX_W && (int64_t)top_k <= VT; }

// ---- launchers (csrc/sample.hip) -------------------------------------------------------------------------------------------------------------
// one sampling step over the whole vocabulary on x [rows, K]: the fused kernel + finish, or the fp32 GEMM + one workgroup per row
size_t sample_gen_bytes(int64_t rows, int K, int64_t VT, bool fused);
int launch_sample_gen(bool fused, const float* x, int64_t rows, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
                      const SampleKey& key, float inv_tau, void* ws, size_t ws_bytes, const SampleOut& o, hipStream_t st);
// the same on the split state h16 [rows][K/8][2 terms][8] the folded LSTM step leaves (gen_fusable(K, VT)): sample_gen_kernel on BeamRowsSplit +
// finish, 4 hq_nvr partials a row
size_t sample_gen_split_bytes(int64_t rows, int K, int64_t VT);
int launch_sample_gen_split(const _Float16* h16, int64_t rows, int K, const float* gen_b, const void* gen_frag, int64_t VT, const SampleKey& key,
                            float inv_tau, void* ws, size_t ws_bytes, const SampleOut& o, hipStream_t st);
// lse NULL: read as 0 (top_val already a log-probability), ids in [0, o.VT + o.CV) -- the copy generator's lists
int launch_sample_topk_select(const float* top_val, const int* top_idx, const float* lse, int64_t rows, int W, const SampleKey& key, float inv_tau,
                              const SampleOut& o, hipStream_t st);
// the decode's first and last launch: the freeze rule's state over R rows; scores / lengths (and the attention rows, QL > 0) in sample order
int launch_sample_init(float* cum, int* fin, int64_t* len, int64_t R, int max_len, hipStream_t st);
int launch_sample_end(const float* cum, const int64_t* len, const float* attn_ws, int64_t B, int N, int max_len, int QL, float* scores, int64_t* lengths,
                      float* attn, hipStream_t st);

}  // namespace nir
