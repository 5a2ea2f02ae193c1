// Sampling decode for HredQS and the session models (include/neuroir_session_sample.h).  Nothing new is drawn: the noise,
// the choice, the freeze rule and the outputs are those of csrc/sample.hip (section 28) with "source row" read as "decode row of the greedy
// decode", and the steps in front of the tail are those of the beams in csrc/beam.hip over R = Bd N un-repeated rows, row r = n Bd + i.  This
// unit holds host code only: the step helpers (CARS: the whole step, CarsRowsStep) come from beam_steps.hpp, the tail (SampleTail: carve, begin,
// draw, end -- the one s2s_sample_decode runs too) and its launchers from sample_tail.hpp, the top-k lists from the public entries
// nir_beam_gen_topk / nir_beam_hredqs_gen_topk.  No sampling loop has a reorder: the state ping-pongs as in s2s_sample_decode,
// step s writes slot s & 1 and reads the other (the first state goes into slot 1).
// Everything is enqueued on the caller's stream: no host synchronisation, no allocation, no atomics.
#include "beam_steps.hpp"
#include "sample_tail.hpp"

namespace nir {

// ---- the decoders without attention (M_MATCH_TENSOR, MNSRF) and HredQS: state buffers + tail -----------------------------------------------------
struct PlainSamplePlan {
    float *h[2], *c[2], *h16[2];
    SampleTail t;
    size_t bytes;
};
static PlainSamplePlan plain_sample_plan(void* ws, size_t cap, int64_t Bd, int H, int64_t VT, int N, int top_k, bool step16, SampleGenForm g) {
    Workspace a(ws, cap);
    PlainSamplePlan p;
    const int64_t R = Bd * N;
    for (int k = 0; k < 2; ++k) { p.h[k] = a.take<float>((size_t)R * H); p.c[k] = a.take<float>((size_t)R * H); }
    for (int k = 0; k < 2; ++k) p.h16[k] = a.take<float>(step16 ? (size_t)R * H : 0);
    p.t.carve(a, R, H, VT, top_k, g);
    p.bytes = align_up(a.off, 256);
    return p;
}
// The loop of both entries below, in the entry's `name`.  begin(p): the first state of every sample row into slot 1 (step16: and its term pairs
// into h16[1]).  Per step: the token-fed LSTM step from slot (s + 1) & 1 into slot s & 1, the draw on the new state.
template <class Begin>
static int plain_sample_decode(const char* name, int64_t Bd, int H, const float* table, int E, const float* w_ih, const float* w_hh, const float* b_ih,
                               const float* b_hh, const float* gate_fold, const void* whh_frag, bool step16, const float* gen_w, const float* gen_b,
                               const void* gen_frag, int64_t VT, SampleGenForm g, const int64_t* tgt2src, int64_t V, int64_t bos, int N, int top_k, float inv_tau,
                               uint64_t seed, int max_len, void* workspace, size_t workspace_bytes, int64_t* predictions, float* token_logprobs,
                               float* scores, int64_t* lengths, hipStream_t st, Begin begin) {
    const int64_t R = Bd * N;
    if (Bd == 0) return 0;                                // nothing to enqueue: no workspace is needed either
    const PlainSamplePlan p = plain_sample_plan(workspace, workspace_bytes, Bd, H, VT, N, top_k, step16, g);
    if (!workspace || p.bytes > workspace_bytes) {
        set_error("%s: workspace too small (%zu < %zu)", name, workspace_bytes, p.bytes);
        return NIR_ERR_WORKSPACE;
    }
    const SampleTail& t = p.t;
    NIR_PROPAGATE(begin(p));
    NIR_PROPAGATE(t.begin(R, bos, max_len, st));
    LstmStepArgs a = beam_lstm_step_args(table, t.tgt, E, w_ih, w_hh, b_ih, b_hh, step16, gate_fold, whh_frag, R, H, p.h, p.c, p.h16);
    SampleOut o = t.out(predictions, token_logprobs, tgt2src, V, VT, Bd, N, max_len);
    for (int step = 0; step < max_len; ++step) {
        const int wr = step & 1, rd = wr ^ 1;
        a.hprev[0] = p.h[rd]; a.cprev[0] = p.c[rd]; a.hnext[0] = p.h[wr]; a.cnext[0] = p.c[wr];
        if (step16) {
            a.h16prev[0] = reinterpret_cast<const _Float16*>(p.h16[rd]);
            a.h16next[0] = reinterpret_cast<_Float16*>(p.h16[wr]);
        }
        NIR_PROPAGATE(launch_lstm_step(a, 1, st));
        o.step = step;
        NIR_PROPAGATE(t.draw(g, p.h[wr], reinterpret_cast<const _Float16*>(p.h16[wr]), R, H, gen_w, gen_b, gen_frag, VT, top_k, sample_key(seed, step, Bd), inv_tau,
                             o, st));
    }
    return t.end(Bd, N, max_len, scores, lengths, st);
}

// ---- CARS: the step of nir_beam_cars_decode over R rows, the tail on p1 ----------------------------------------------------------------------------------
struct CarsSamplePlan {
    CarsRowsStep s;
    SampleTail t;
    size_t bytes;
};
static CarsSamplePlan cars_sample_plan(void* ws, size_t cap, int64_t rows_src, int64_t Bd, int QL, int N, int top_k, const nir_cars_decoder_weights* w,
                                       bool fused) {
    Workspace a(ws, cap);
    CarsSamplePlan p;
    p.s.carve(a, rows_src, Bd * N, QL, w);
    p.t.carve(a, Bd * N, w->P, w->VT, top_k, fused ? SAMPLE_GEN_FUSED : SAMPLE_GEN_PLAIN);
    p.bytes = align_up(a.off, 256);
    return p;
}

static bool sess_rows_ok(int64_t Bd, int N) { return Bd >= 0 && Bd < 0x7FFFFFFFLL && N >= 1 && Bd * (int64_t)N < 0x7FFFFFFFLL; }

}  // namespace nir

extern "C" size_t nir_sample_hredqs_gen_workspace_bytes(int64_t rows, int K, int64_t VT) {
    using namespace nir;
    if (rows <= 0 || rows >= 0x7FFFFFFFLL || !gen_fusable(K, VT)) return 0;
    return sample_gen_split_bytes(rows, K, VT);
}

extern "C" int nir_sample_hredqs_gen(const void* h16, int64_t rows, int64_t nsrc, int K, const float* gen_b, const void* gen_frag, int64_t VT,
                                     float inv_temperature, uint64_t seed, int64_t step, void* workspace, size_t workspace_bytes, int32_t* token,
                                     float* logp, float* lse, nir_stream_t stream) {
    using namespace nir;
    NIR_REQUIRE(h16 && gen_frag && token && logp, "sample_hredqs_gen: null pointer");
    NIR_REQUIRE(sample_key_ok(step, nsrc, rows), "sample_hredqs_gen: step outside [0, 2^32), nsrc < 1 or rows outside [0, 2^31)");
    NIR_REQUIRE(gen_fusable(K, VT), "sample_hredqs_gen: K must be a multiple of 32 in [32, 1024] and 0 < VT < 2^31 - 16");
    NIR_REQUIRE(sample_tau_ok(inv_temperature), "sample_hredqs_gen: inv_temperature must be finite and > 0");
    if (rows == 0) return 0;
    if (!workspace || workspace_bytes < sample_gen_split_bytes(rows, K, VT)) {
        set_error("sample_hredqs_gen: workspace null or too small");
        return NIR_ERR_WORKSPACE;
    }
    const SampleOut o{token, logp, lse, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, VT, nsrc, 1, 0, 1};
    return launch_sample_gen_split((const _Float16*)h16, rows, K, gen_b, gen_frag, VT, sample_key(seed, step, nsrc), inv_temperature, workspace,
                                   workspace_bytes, o, (hipStream_t)stream);
}

extern "C" size_t nir_sample_hredqs_decode_workspace_bytes(int64_t B, int64_t S, int N, int top_k, int max_len, const nir_hredqs_decoder_weights* w) {
    using namespace nir;
    if (!hq_weights_ok(w) || B < 0 || S < 0 || B >= 0x7FFFFFFFLL || S >= 0x7FFFFFFFLL || max_len <= 0 || !sample_dims_ok(N, top_k, w->VT) ||
        !sess_rows_ok(B * S, N))
        return 0;
    const bool fast = hq_fast(w);
    return plain_sample_plan(nullptr, 0, B * S, w->H, w->VT, N, top_k, fast, fast ? SAMPLE_GEN_SPLIT : SAMPLE_GEN_PLAIN).bytes;
}

extern "C" int nir_sample_hredqs_decode(const float* h_steps, const float* c_steps, int64_t B, int64_t S, const float* table, int64_t V, int E,
                                        const int64_t* tgt2src, int64_t bos, int max_len, const nir_hredqs_decoder_weights* w, int N, int top_k,
                                        float inv_temperature, uint64_t seed, void* workspace, size_t workspace_bytes, int64_t* predictions,
                                        float* token_logprobs, float* scores, int64_t* lengths, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(h_steps && c_steps && table && w && predictions && token_logprobs && scores && lengths, "sample_hredqs_decode: null pointer");
    NIR_REQUIRE(hq_weights_ok(w), "sample_hredqs_decode: decoder weights incomplete, H not a multiple of 4 or VT outside (0, 2^31 - 16)");
    NIR_REQUIRE(B >= 0 && S >= 0 && max_len > 0 && V > 0 && E > 0 && E % 4 == 0, "sample_hredqs_decode: bad dims");
    NIR_REQUIRE(bos >= 0 && bos < V, "sample_hredqs_decode: BOS id outside the vocabulary");
    NIR_REQUIRE((w->rnn_gate_fold == nullptr) == (w->rnn_whh_frag == nullptr), "sample_hredqs_decode: rnn_gate_fold and rnn_whh_frag come together");
    NIR_REQUIRE(sample_dims_ok(N, top_k, w->VT), "sample_hredqs_decode: N < 1, or top_k outside 0 .. %d or above the target vocabulary", NIR_BEAM_MAX_W);
    NIR_REQUIRE(sample_tau_ok(inv_temperature), "sample_hredqs_decode: inv_temperature must be finite and > 0");
    NIR_REQUIRE(B < 0x7FFFFFFFLL && S < 0x7FFFFFFFLL && sess_rows_ok(B * S, N), "sample_hredqs_decode: too many decode rows");
    const int H = w->H;
    const int64_t Bd = B * S, R = Bd * N;
    const bool fast = hq_fast(w);
    return plain_sample_decode("sample_hredqs_decode", Bd, H, table, E, w->rnn_wih, w->rnn_whh, w->rnn_bih, w->rnn_bhh, w->rnn_gate_fold, w->rnn_whh_frag, fast,
                               w->gen_w, w->gen_b, w->gen_frag, w->VT, fast ? SAMPLE_GEN_SPLIT : SAMPLE_GEN_PLAIN, tgt2src, V, bos, N, top_k, inv_temperature, seed,
                               max_len, workspace, workspace_bytes, predictions, token_logprobs, scores, lengths, st, [&](const PlainSamplePlan& p) {
                                   // pairing, repeat and split in one launch: every sample of decode row i starts from step i / B of session i % B
                                   return launch_hq_beam_begin(h_steps, c_steps, B, S, H, R, p.h[1], p.c[1],
                                                               fast ? reinterpret_cast<_Float16*>(p.h16[1]) : nullptr, st);
                               });
}

extern "C" size_t nir_sample_plain_decode_workspace_bytes(int64_t Bd, int H, int64_t VT, int N, int top_k, int max_len, int folded, int fused) {
    using namespace nir;
    if (H <= 0 || H % 4 || VT <= 0 || VT >= 0x7FFFFFF0LL || max_len <= 0 || !sample_dims_ok(N, top_k, VT) || !sess_rows_ok(Bd, N)) return 0;
    const bool fuse = fused && gen_fusable(H, VT) && !tun(g_tun.exact_f32);
    return plain_sample_plan(nullptr, 0, Bd, H, VT, N, top_k, folded && H % 32 == 0 && !tun(g_tun.exact_f32), fuse ? SAMPLE_GEN_FUSED : SAMPLE_GEN_PLAIN).bytes;
}

extern "C" int nir_sample_plain_decode(const float* dec_h, const float* dec_c, int64_t Bd, int H, const float* table, int64_t V, int E, const float* w_ih,
                                       const float* w_hh, const float* b_ih, const float* b_hh, const float* gen_w, const float* gen_b, int64_t VT,
                                       const int64_t* tgt2src, int64_t bos, int max_len, const float* gate_fold, const void* whh_frag,
                                       const void* gen_frag, int N, int top_k, float inv_temperature, uint64_t seed, void* workspace,
                                       size_t workspace_bytes, int64_t* predictions, float* token_logprobs, float* scores, int64_t* lengths,
                                       nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(dec_h && dec_c && table && w_ih && w_hh && b_ih && b_hh && gen_w && predictions && token_logprobs && scores && lengths,
                "sample_plain_decode: null pointer");
    NIR_REQUIRE(Bd >= 0 && H > 0 && E > 0 && V > 0 && VT > 0 && max_len > 0 && E % 4 == 0 && H % 4 == 0, "sample_plain_decode: bad dims");
    NIR_REQUIRE(bos >= 0 && bos < V, "sample_plain_decode: BOS id outside the vocabulary");
    NIR_REQUIRE(sample_dims_ok(N, top_k, VT), "sample_plain_decode: N < 1, or top_k outside 0 .. %d or above the target vocabulary", NIR_BEAM_MAX_W);
    NIR_REQUIRE(sample_tau_ok(inv_temperature), "sample_plain_decode: inv_temperature must be finite and > 0");
    NIR_REQUIRE(sess_rows_ok(Bd, N) && VT < 0x7FFFFFF0LL, "sample_plain_decode: too many decode rows or target tokens");
    const int64_t R = Bd * N;
    const bool step16 = gate_fold && whh_frag && H % 32 == 0 && !tun(g_tun.exact_f32), fused = s2s_gen_fused(gen_frag, H, VT);
    return plain_sample_decode("sample_plain_decode", Bd, H, table, E, w_ih, w_hh, b_ih, b_hh, gate_fold, whh_frag, step16, gen_w, gen_b, gen_frag, VT,
                               fused ? SAMPLE_GEN_FUSED : SAMPLE_GEN_PLAIN, tgt2src, V, bos, N, top_k, inv_temperature, seed, max_len, workspace, workspace_bytes,
                               predictions, token_logprobs, scores, lengths, st, [&](const PlainSamplePlan& p) {
                                   return launch_beam_repeat(dec_h, dec_c, Bd, R, H, p.h[1], p.c[1], step16 ? p.h16[1] : nullptr, nullptr, nullptr, st);
                               });
}

extern "C" size_t nir_sample_cars_decode_workspace_bytes(int64_t rows_src, int64_t Bd, int QL, int N, int top_k, int max_len,
                                                         const nir_cars_decoder_weights* w, int fused) {
    using namespace nir;
    if (!cars_beam_weights_ok(w) || rows_src < 0 || QL <= 0 || max_len <= 0 || w->VT >= 0x7FFFFFF0LL || !sample_dims_ok(N, top_k, w->VT) || !sess_rows_ok(Bd, N))
        return 0;
    return cars_sample_plan(nullptr, 0, rows_src, Bd, QL, N, top_k, w, fused && gen_fusable(w->P, w->VT) && !tun(g_tun.exact_f32)).bytes;
}

extern "C" int nir_sample_cars_decode(const float* dec_h, const float* dec_c, const float* encoded_source, const int64_t* source_len, int64_t rows_src,
                                      int QL, const int64_t* rowmap, int64_t Bd, const float* session_cat, const float* table, int64_t V, int E,
                                      const int64_t* tgt2src, int64_t bos, int max_len, const nir_cars_decoder_weights* w, const void* gen_frag, int N,
                                      int top_k, float inv_temperature, uint64_t seed, void* workspace, size_t workspace_bytes, int64_t* predictions,
                                      float* token_logprobs, float* scores, int64_t* lengths, nir_stream_t stream) {
    using namespace nir;
    hipStream_t st = (hipStream_t)stream;
    NIR_REQUIRE(dec_h && dec_c && encoded_source && source_len && rowmap && table && w && predictions && token_logprobs && scores && lengths,
                "sample_cars_decode: null pointer");
    NIR_REQUIRE(cars_beam_weights_ok(w), "sample_cars_decode: null weight pointer or bad dims (HD, DQ, P multiples of 4)");
    NIR_REQUIRE(rows_src > 0 && Bd >= 0 && QL > 0 && max_len > 0 && V > 0 && E > 0 && E % 4 == 0, "sample_cars_decode: bad dims");
    NIR_REQUIRE(w->KS == 0 || (session_cat && w->sess_w), "sample_cars_decode: session representation / packed projector missing");
    NIR_REQUIRE(bos >= 0 && bos < V, "sample_cars_decode: BOS id outside the vocabulary");
    NIR_REQUIRE(sample_dims_ok(N, top_k, w->VT), "sample_cars_decode: N < 1, or top_k outside 0 .. %d or above the target vocabulary", NIR_BEAM_MAX_W);
    NIR_REQUIRE(sample_tau_ok(inv_temperature), "sample_cars_decode: inv_temperature must be finite and > 0");
    NIR_REQUIRE(sess_rows_ok(Bd, N) && w->VT < 0x7FFFFFF0LL, "sample_cars_decode: too many decode rows or target tokens");
    const int P = w->P;
    const int64_t R = Bd * N, VT = w->VT;
    const bool fused = s2s_gen_fused(gen_frag, P, VT);
    if (Bd == 0) return 0;                                // nothing to enqueue: no workspace is needed either
    CarsSamplePlan p = cars_sample_plan(workspace, workspace_bytes, rows_src, Bd, QL, N, top_k, w, fused);
    const SampleTail& t = p.t;
    if (!workspace || p.bytes > workspace_bytes) {
        set_error("sample_cars_decode: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
        return NIR_ERR_WORKSPACE;
    }
    NIR_PROPAGATE(p.s.prepare(dec_h, dec_c, encoded_source, source_len, rows_src, rowmap, Bd, session_cat, table, t.tgt, E, 1, st,
                              [&] { return t.begin(R, bos, max_len, st); }));
    SampleOut o = t.out(predictions, token_logprobs, tgt2src, V, VT, Bd, N, max_len);
    const SampleGenForm g = fused ? SAMPLE_GEN_FUSED : SAMPLE_GEN_PLAIN;
    for (int step = 0; step < max_len; ++step) {
        const int wr = step & 1;
        NIR_PROPAGATE(p.s.step(wr ^ 1, wr));
        o.step = step;
        NIR_PROPAGATE(t.draw(g, p.s.p1, nullptr, R, P, w->pred2_w, nullptr, gen_frag, VT, top_k, sample_key(seed, step, Bd), inv_temperature, o, st));
    }
    return t.end(Bd, N, max_len, scores, lengths, st);
}
