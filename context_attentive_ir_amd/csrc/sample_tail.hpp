// The sampling tail as the decodes see it (csrc/sample.hip, csrc/session_sample.hip; DESIGN.md sections 28, 29 and 33): the key of the noise, where a
// row's choice goes, the argument checks, the launchers, and SampleTail -- the tail's part of a workspace plan with the launches on it, shared by
// all five sampling decodes (Seq2seq, ACG, HredQS, plain, CARS).  The kernels live in csrc/sample.hip; these are their host-side launchers.
#pragma once
#include <cmath>
#include "decode_common.hpp"

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

// ---- the tail of every sampling decode, on the host -----------------------------------------------------------------------------------------------
// where the tail reads a step's rows from, and which generator it runs on them
enum SampleGenForm { SAMPLE_GEN_PLAIN = 0, SAMPLE_GEN_FUSED = 1, SAMPLE_GEN_SPLIT = 2 };     // fp32 rows + GEMM; fp32 rows, fused; the split state, fused

// The tail's part of a workspace plan over R sample rows (row r = n nsrc + b), behind a decoder's step buffers, and the launches on it: begin,
// the per-step draw in its plain, fused, split and top-k forms, end.
struct SampleTail {
    int64_t* tgt;                                     // [R] the ids the next step reads
    void* gen;                                        // the generator's workspace
    size_t gen_bytes;
    float *tval, *lse;                                // top_k > 0, own lists: the rows' lists [R, top_k] and lse [R]
    int* tidx;
    float* cum;                                       // [R] the state of the freeze rule
    int* fin;
    int64_t* len;
    // gen_bytes_: the generator's byte count; own_lists: the tail keeps the top-k lists (the copy generator's forms keep theirs inside gen)
    void carve(Workspace& a, int64_t R, int top_k, size_t gen_bytes_, bool own_lists) {
        tgt = a.take<int64_t>((size_t)R);
        gen_bytes = gen_bytes_;
        gen = a.take<char>(gen_bytes);
        tval = a.take<float>(own_lists ? (size_t)R * top_k : 0);
        tidx = a.take<int>(own_lists ? (size_t)R * top_k : 0);
        lse = a.take<float>(own_lists && top_k > 0 ? (size_t)R : 0);
        cum = a.take<float>((size_t)R);
        fin = a.take<int>((size_t)R);
        len = a.take<int64_t>((size_t)R);
    }
    // the tail's own generator on rows of K values, in form g
    void carve(Workspace& a, int64_t R, int K, int64_t VT, int top_k, SampleGenForm g) {
        carve(a, R, top_k,
              R == 0      ? 0
              : top_k > 0 ? (g == SAMPLE_GEN_SPLIT ? nir_beam_hredqs_gen_topk_workspace_bytes(R, K, VT, top_k)
                                                   : nir_beam_gen_topk_workspace_bytes(R, K, VT, top_k, g == SAMPLE_GEN_FUSED))
              : g == SAMPLE_GEN_SPLIT ? sample_gen_split_bytes(R, K, VT)
                                      : sample_gen_bytes(R, K, VT, g == SAMPLE_GEN_FUSED),
              true);
    }
    int init(int64_t R, int max_len, hipStream_t st) const { return launch_sample_init(cum, fin, len, R, max_len, st); }
    // the BOS fill and init (a stepper fills tgt with its own launch and calls init alone)
    int begin(int64_t R, int64_t bos, int max_len, hipStream_t st) const {
        NIR_PROPAGATE(launch_fill_i64(tgt, bos, R, st));
        return init(R, max_len, st);
    }
    // e2s / CV: the copy generator's dictionary slots (SampleOut)
    SampleOut out(int64_t* predictions, float* token_logprobs, const int64_t* tgt2src, int64_t V, int64_t VT, int64_t Bd, int N, int max_len,
                  const int64_t* e2s = nullptr, int CV = 0) const {
        return SampleOut{nullptr, nullptr, nullptr, fin, cum, len, predictions, token_logprobs, tgt, tgt2src, V, VT, Bd, N, 0, max_len, e2s, CV};
    }
    // one step's draw for all R rows: x [R, K] fp32 (PLAIN, FUSED) or h16 [R][K/8][2][8] (SPLIT)
    int draw(SampleGenForm g, const float* x, const _Float16* h16, int64_t R, int K, const float* gen_w, const float* gen_b, const void* gen_frag, int64_t VT,
             int top_k, const SampleKey& key, float inv_tau, const SampleOut& o, hipStream_t st) const {
        if (top_k > 0) {
            const int rc = g == SAMPLE_GEN_SPLIT
                               ? nir_beam_hredqs_gen_topk(h16, R, K, gen_b, gen_frag, VT, top_k, gen, gen_bytes, tval, tidx, lse, (nir_stream_t)st)
                               : nir_beam_gen_topk(x, R, K, gen_w, gen_b, g == SAMPLE_GEN_FUSED ? gen_frag : nullptr, VT, top_k, gen, gen_bytes, tval, tidx, lse,
                                                   (nir_stream_t)st);
            if (rc != 0) return rc;
            return launch_sample_topk_select(tval, tidx, lse, R, top_k, key, inv_tau, o, st);
        }
        if (g == SAMPLE_GEN_SPLIT) return launch_sample_gen_split(h16, R, K, gen_b, gen_frag, VT, key, inv_tau, gen, gen_bytes, o, st);
        return launch_sample_gen(g == SAMPLE_GEN_FUSED, x, R, K, gen_w, gen_b, gen_frag, VT, key, inv_tau, gen, gen_bytes, o, st);
    }
    // scores / lengths in sample order; attn_ws [max_len][R][QL] given: and the attention rows of every step
    int end(int64_t Bd, int N, int max_len, float* scores, int64_t* lengths, hipStream_t st, const float* attn_ws = nullptr, int QL = 0,
            float* attentions = nullptr) const {
        return launch_sample_end(cum, len, attn_ws, Bd, N, max_len, QL, scores, lengths, attentions, st);
    }
};

}  // namespace nir
