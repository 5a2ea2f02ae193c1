"""GPU (-m gpu): folded-embedding BiLSTM (csrc/lstm_fold.hip) and the CARS encoders built on it.

fp32 folded path = the parity path: same 1e-4 bar on scores as everything else (observed ~1e-6).
bf16 path (BASELINE config 5): bf16 cannot meet 1e-4.  Its ACHIEVED error against the oracle is measured by tools/bf16_error_survey.py over the
shapes used here (round 5, gpurun_out/bf16_error_survey_r05.json -> profiles/r05_bf16_error_survey.json): max |score - oracle| 5.4e-4, max
|softmax prob diff| 3.3e-5, MAP delta 0 on every shape (rows reorder only where the oracle's own gap is < 1.3e-4).  The bounds below are
<= 2x those maxima: |score - oracle| <= BF16_SCORE_TOL on raw click scores, |prob diff| <= BF16_PROB_TOL, identical order wherever the oracle
separates neighbours by more than twice the bound, and MAP@10 EQUAL to the oracle's on 10-candidate sets."""
import numpy as np
import pytest
import torch

from helpers import build_model, cpu_state_dict
from oracle import neuroir_cpu as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16_SCORE_TOL = 1.1e-3
BF16_PROB_TOL = 7e-5
BF16_MAP_TOL = 5e-3          # candidate sets wider than 10 (near-ties among 50 random-weight scores); 10-candidate sets: equality


def _close(a, b, tol):
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().float().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=0, atol=tol)


@pytest.mark.parametrize("H,M,T_,V", [(128, 40, 12, 500), (128, 1, 1, 50), (70, 33, 20, 300), (15, 50, 6, 100), (96, 21, 290, 800),
                                      (40, 17, 11, 64), (8, 5, 3, 20), (100, 35, 64, 1000)])
def test_bilstm_folded_f32_vs_oracle(H, M, T_, V):
    """nir_lstm_fold_table + nir_bilstm_folded_fwd against the oracle's embedding lookup + RNNEncoder, ragged lengths,
    partial workgroups (M % 16 != 0), hidden sizes that do not fill the last MFMA tile."""
    from context_attentive_ir_amd import lib
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.encoders import RNNEncoder
    from context_attentive_ir_amd.encoders.rnn_encoder import lstm_cat_weights
    E = 300
    enc = fill_module_(RNNEncoder("LSTM", E, True, 1, 2 * H), seed=5).eval()
    g = torch.Generator().manual_seed(H * 7 + M)
    table = (torch.rand(V, E, generator=g) - 0.5)
    table[0].zero_()
    lens = torch.randint(1, T_ + 1, (M,), generator=g); lens[0] = T_
    ids = torch.randint(1, V, (M, T_), generator=g)
    ids[torch.arange(T_)[None] >= lens[:, None]] = 0
    sd = {"e." + k: v for k, v in enc.state_dict().items()}
    _, ref = O.rnn_encode(sd, "e", table[ids], lens)
    wih, whh, bih, bhh = (t.detach().float().contiguous().to(DEV) for t in lstm_cat_weights(enc.rnns[0]))
    folded = lib.fold_lstm_table(table.to(DEV), wih, bih, bhh, H, 2, "f32")
    out = torch.empty(M, T_, 2 * H, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    idd, ld = ids.to(DEV), lens.to(DEV)
    lib.check(lib.load().nir_bilstm_folded_fwd(lib.ptr(folded), lib.DTYPE_F32, lib.ptr(idd), lib.ptr(ld), lib.ptr(whh), lib.ptr(out),
                                               lib.ptr(err), M, V, T_, H, 2, lib.stream()), "folded")
    _close(out, ref, 2e-5)
    assert int(err.item()) == 0


@pytest.mark.parametrize("H,M,T_,V", [(128, 40, 12, 500), (128, 19, 64, 900), (64, 33, 20, 300), (96, 21, 30, 200), (32, 5, 9, 50)])
def test_bilstm_folded_bf16_vs_oracle(H, M, T_, V):
    """bf16 folded table + bf16 MFMA recurrence: hidden states within 3e-2 of the fp32 oracle (|h| < 1)."""
    from context_attentive_ir_amd import lib
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.encoders import RNNEncoder
    from context_attentive_ir_amd.encoders.rnn_encoder import lstm_cat_weights
    E = 300
    enc = fill_module_(RNNEncoder("LSTM", E, True, 1, 2 * H), seed=5).eval()
    g = torch.Generator().manual_seed(H * 7 + M)
    table = (torch.rand(V, E, generator=g) - 0.5)
    table[0].zero_()
    lens = torch.randint(1, T_ + 1, (M,), generator=g); lens[0] = T_
    ids = torch.randint(1, V, (M, T_), generator=g)
    ids[torch.arange(T_)[None] >= lens[:, None]] = 0
    sd = {"e." + k: v for k, v in enc.state_dict().items()}
    _, ref = O.rnn_encode(sd, "e", table[ids], lens)
    wih, whh, bih, bhh = (t.detach().float().contiguous().to(DEV) for t in lstm_cat_weights(enc.rnns[0]))
    folded = lib.fold_lstm_table(table.to(DEV), wih, bih, bhh, H, 2, "bf16")
    out = torch.empty(M, T_, 2 * H, device=DEV)
    idd, ld = ids.to(DEV), lens.to(DEV)
    lib.check(lib.load().nir_bilstm_folded_fwd(lib.ptr(folded), lib.DTYPE_BF16, lib.ptr(idd), lib.ptr(ld), lib.ptr(whh), lib.ptr(out),
                                               None, M, V, T_, H, 2, lib.stream()), "folded bf16")
    _close(out, ref, 3e-2)
    assert float((out.cpu() - ref).abs().mean()) < 4e-3


def test_folded_matches_unfolded_cars_encoders():
    """CARS.encode / encode_document: folded path (default in eval) vs the per-batch gather-GEMM path, fp32."""
    from context_attentive_ir_amd import synth
    V = 3000
    m = build_model("CARS", vocab=V, device=DEV)
    ex = {k: v.to(DEV) for k, v in synth.session_batch(3, 4, 9, 6, 41, V, seed=11, full_length=False).items()}
    assert m.fold_embeddings
    p1, e1, _ = m.encode(ex["source_words"], ex["source_lens"])
    d1 = m.encode_document(ex["document_words"], ex["document_lens"])
    m.fold_embeddings = False
    p0, e0, _ = m.encode(ex["source_words"], ex["source_lens"])
    d0 = m.encode_document(ex["document_words"], ex["document_lens"])
    _close(e1, e0, 5e-6); _close(p1, p0, 5e-6); _close(d1, d0, 5e-6)


def test_folded_table_follows_weight_updates():
    """The folded tables are re-derived when the embedding table or the LSTM weights change (lib.PackCache keys)."""
    from context_attentive_ir_amd import synth
    V = 500
    m = build_model("CARS", vocab=V, device=DEV)
    ex = {k: v.to(DEV) for k, v in synth.session_batch(2, 2, 3, 4, 9, V, seed=3).items()}
    a = m.encode_document(ex["document_words"], ex["document_lens"]).clone()
    with torch.no_grad():
        m.embedder.word_embeddings.table.mul_(0.5)
    b = m.encode_document(ex["document_words"], ex["document_lens"]).clone()
    m.fold_embeddings = False
    c = m.encode_document(ex["document_words"], ex["document_lens"])
    assert float((a - b).abs().max()) > 1e-3
    _close(b, c, 5e-6)


def test_out_of_vocabulary_id_raises_index_error():
    """nn.Embedding raises IndexError for id >= V (reference); the folded kernels clamp + flag, check_ids() raises."""
    from context_attentive_ir_amd import synth
    V = 200
    m = build_model("CARS", vocab=V, device=DEV)
    ex = {k: v.to(DEV) for k, v in synth.session_batch(2, 2, 3, 4, 9, V, seed=3).items()}
    m.encode_document(ex["document_words"], ex["document_lens"])
    m.check_ids()
    bad = ex["document_words"].clone()
    bad[0, 0, 0, 0] = V + 5
    m.encode_document(bad, ex["document_lens"])
    with pytest.raises(IndexError):
        m.check_ids()
    m.encode_document(ex["document_words"], ex["document_lens"])
    m.check_ids()      # flag was cleared


@pytest.mark.parametrize("B,S,N,QL,DL", [(4, 7, 10, 6, 64), (2, 3, 50, 6, 64)])
def test_cars_bf16_scores_and_map(B, S, N, QL, DL):
    """BASELINE config 5 precision: bf16 folded tables + bf16 recurrence against the fp32 oracle."""
    from context_attentive_ir_amd import synth
    from context_attentive_ir_amd.eval import ltorank
    V = 3000
    m = build_model("CARS", vocab=V, device=DEV)
    m.compute_dtype = "bf16"
    ex = synth.session_batch(B, S, N, QL, DL, V, seed=B + S, full_length=False)
    sd = cpu_state_dict(m)
    ref = O.cars_scores(sd, ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"], ex["document_labels"])
    dex = {k: v.to(DEV) for k, v in ex.items()}
    pooled, _, _ = m.encode(dex["source_words"], dex["source_lens"])
    s, _, _ = m.rank_document(pooled, dex["document_words"], dex["document_lens"], dex["document_labels"])
    s = s.cpu()
    assert float((s - ref).abs().max()) <= BF16_SCORE_TOL, float((s - ref).abs().max())
    _close(torch.softmax(s, -1), torch.softmax(ref, -1), BF16_PROB_TOL)
    # rank agreement wherever the oracle separates neighbours by more than twice the bound
    lab = ex["document_labels"].reshape(-1, N).numpy()
    r_ref, r_got = ref.reshape(-1, N).numpy(), s.reshape(-1, N).numpy()
    srt = np.sort(r_ref, 1)
    safe = (np.diff(srt, axis=1).min(1) > 2 * BF16_SCORE_TOL)
    if safe.any():
        assert (np.argsort(-r_ref[safe], 1) == np.argsort(-r_got[safe], 1)).all()
    map_ref = ltorank.MAP(np.argsort(-r_ref, 1, kind="stable"), lab)
    map_got = ltorank.MAP(np.argsort(-r_got, 1, kind="stable"), lab)
    if N == 10:
        assert map_ref == map_got, (map_ref, map_got)              # MAP@10 parity (BASELINE metric): equality
    else:
        assert abs(map_ref - map_got) <= BF16_MAP_TOL, (map_ref, map_got)


@pytest.mark.parametrize("S,N,QL,DL", [(3, 5, 4, 64), (2, 7, 8, 16), (4, 3, 16, 32), (1, 2, 4, 4)])
def test_fused_attention_pooling_matches_layer_chain_and_oracle(S, N, QL, DL):
    """The fused attention-pooling kernel (csrc/cars_attn.hip; sequence lengths 4 / 8 / 16 / 32 / 64 rows per tile, ragged lengths,
    a partial last tile) against the GEMM + pooling chain (tunable attn_unfused) and the oracle's CARS.encode / encode_document."""
    from context_attentive_ir_amd import lib, synth
    V, B = 2000, 3
    m = build_model("CARS", vocab=V, device=DEV)
    ex = synth.session_batch(B, S, N, QL, DL, V, seed=QL + DL, full_length=False)
    exd = {k: v.to(DEV) for k, v in ex.items()}
    assert m._enc_weights("d").struct.attn_frag and m._enc_weights("q").struct.attn_frag
    p1, e1, _ = m.encode(exd["source_words"], exd["source_lens"])
    d1 = m.encode_document(exd["document_words"], exd["document_lens"])
    with lib.tunable("attn_unfused", 1, 0):
        p0, e0, _ = m.encode(exd["source_words"], exd["source_lens"])
        d0 = m.encode_document(exd["document_words"], exd["document_lens"])
    # (twice the worst deviation measured on the MI355X over the four shapes: 5.96e-8 for the queries, 1.49e-7 for the documents)
    _close(p1, p0, 1.2e-7); _close(d1, d0, 3e-7); _close(e1, e0, 0)
    sd = cpu_state_dict(m)
    pq, _ = O.cars_encode(sd, ex["source_words"], ex["source_lens"])
    _close(p1, pq, 2.4e-7)                               # against the oracle: measured worst 1.19e-7 (queries), 1.49e-7 (documents)
    _close(d1, O.cars_encode_document(sd, ex["document_words"], ex["document_lens"]), 3e-7)


@pytest.mark.parametrize("S,N,QL,DL", [(3, 9, 4, 64), (2, 5, 8, 16), (5, 3, 16, 32), (1, 2, 4, 4)])
def test_attention_pooling_pipeline_kernel(S, N, QL, DL):
    """The persistent role-specialised attention-pooling kernel (bench-size document encoders select it by tile count; here it is forced,
    tunable attn_unfused_pipe = 2): more tiles than / fewer tiles than workgroups, ragged lengths, a partial last tile."""
    from context_attentive_ir_amd import lib, synth
    V, B = 2000, 4
    m = build_model("CARS", vocab=V, device=DEV)
    ex = {k: v.to(DEV) for k, v in synth.session_batch(B, S, N, QL, DL, V, seed=QL * DL, full_length=False).items()}
    with lib.tunable("attn_unfused", 1, 0):
        p0, _, _ = m.encode(ex["source_words"], ex["source_lens"])
        d0 = m.encode_document(ex["document_words"], ex["document_lens"])
    with lib.tunable("attn_unfused_pipe", 2, 0):
        p1, _, _ = m.encode(ex["source_words"], ex["source_lens"])
        d1 = m.encode_document(ex["document_words"], ex["document_lens"])       # H = 128: the recurrence hands its term pairs over (mode 2)
        with lib.tunable("attn_fp32_rows", 1, 0):
            d2 = m.encode_document(ex["document_words"], ex["document_lens"])   # fp32 rows, split again by the IO waves (mode 0)
    # (twice the worst deviation measured on the MI355X over the four shapes: 8.94e-8, 1.19e-7 and 1.49e-7)
    _close(p1, p0, 1.8e-7); _close(d1, d0, 2.4e-7); _close(d2, d0, 3e-7)
    assert not torch.equal(d1, d2)                       # two different roundings of the residual term (nearest vs toward zero): both ran


def test_recurrence_hands_term_pairs_to_attention_pipeline_vs_oracle():
    """A document block large enough for the pipeline to be selected by tile count (608 documents x 64 steps = 608 tiles >= 2 x 256 CUs), ragged
    lengths: lstm16_pt_h2_kernel<4,4,8> writes every h_t as [4 x leading fp16 term | 4 x residual term] per group of 4 units and
    attn_pool_pipe_kernel<false,2> stages those 16-byte groups straight into its LDS planes.  pooled_docs against the ORACLE at 3.9e-7
    (|pooled| < 1), and the raw hand-over buffer decodes to the fp32 states of the plain output (2^-22 relative to |h| < 1)."""
    from context_attentive_ir_amd import lib
    V, M, T_ = 3000, 608, 64
    m = build_model("CARS", vocab=V, device=DEV)
    g = torch.Generator().manual_seed(77)
    ids = torch.randint(4, V, (M, T_), generator=g)
    lens = torch.randint(1, T_ + 1, (M,), generator=g)
    lens[:40] = T_
    ids = torch.where(torch.arange(T_)[None, :] < lens[:, None], ids, torch.zeros_like(ids))
    sd = cpu_state_dict(m)
    ref = O.cars_encode_document(sd, ids.view(1, 1, M, T_), lens.view(1, 1, M)).view(M, -1)
    got = m.encode_document(ids.view(1, 1, M, T_).to(DEV), lens.view(1, 1, M).to(DEV)).view(M, -1).cpu()
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=3.9e-7)             # measured worst 1.94e-7, both row formats
    with lib.tunable("attn_fp32_rows", 1, 0):
        got0 = m.encode_document(ids.view(1, 1, M, T_).to(DEV), lens.view(1, 1, M).to(DEV)).view(M, -1).cpu()
    np.testing.assert_allclose(got0.numpy(), ref.numpy(), rtol=0, atol=3.9e-7)
    assert not torch.equal(got, got0)
    # the hand-over format itself, through the C-ABI recurrence entry (plain fp32 output) against the decode of what the pipeline reads
    from context_attentive_ir_amd.encoders.rnn_encoder import lstm_cat_weights
    wih, whh, bih, bhh = [t.detach().contiguous() for t in lstm_cat_weights(m.document_encoder.encoder.rnns[0])]
    folded = lib.fold_lstm_table(m.embedder.word_embeddings.table.detach(), wih, bih, bhh, 128, 2, "f32")
    out = torch.empty(M, T_, 256, device=DEV)
    lib.check(lib.load().nir_bilstm_folded_fwd(lib.ptr(folded), lib.DTYPE_F32, lib.ptr(ids.to(DEV)), lib.ptr(lens.to(DEV)), lib.ptr(whh), lib.ptr(out), None,
                                                M, V, T_, 128, 2, lib.stream()), "folded")
    _, enc = O.rnn_encode(sd, "document_encoder.encoder", O.embed(sd, "embedder.word_embeddings", ids), lens)
    np.testing.assert_allclose(out.cpu().numpy(), enc.detach().numpy(), rtol=0, atol=2e-5)


def test_bilstm_folded_four_wave_variant_matches():
    """H = 70: the 4-wave x 5-tile workgroup form (selected by workgroup count; forced here with tunable lstm_s = 2) against the
    16-wave form (lstm_s = 1): the same arithmetic in another wave layout (agreement to rounding, 1e-6)."""
    from context_attentive_ir_amd import lib
    H, M, T_, V = 70, 37, 21, 300
    g = torch.Generator().manual_seed(5)
    x = torch.randn(V, 40, generator=g).to(DEV)
    lstm = torch.nn.LSTM(40, H, bidirectional=True, batch_first=True).to(DEV)
    from context_attentive_ir_amd.encoders.rnn_encoder import lstm_cat_weights
    wih, whh, bih, bhh = [t.detach().contiguous() for t in lstm_cat_weights(lstm)]
    folded = lib.fold_lstm_table(x, wih, bih, bhh, H, 2, "f32")
    ids = torch.randint(0, V, (M, T_), generator=g).to(DEV)
    lens = torch.randint(1, T_ + 1, (M,), generator=g).to(DEV)
    outs = []
    for sel in (1, 2):
        out = torch.empty(M, T_, 2 * H, device=DEV)
        with lib.tunable("lstm_s", sel, 0):
            lib.check(lib.load().nir_bilstm_folded_fwd(lib.ptr(folded), lib.DTYPE_F32, lib.ptr(ids), lib.ptr(lens), lib.ptr(whh), lib.ptr(out),
                                                        None, M, V, T_, H, 2, lib.stream()), "folded")
        outs.append(out)
    _close(outs[0], outs[1], 1e-6)


def test_bilstm_folded_h128_matches_oracle():
    """H = 128: the folded recurrence (lstm16_pt_h2_kernel<4,4,8>) against the oracle: ragged lengths, a one-step sequence, a partial last
    workgroup, both directions, no out-of-range weight flagged."""
    from context_attentive_ir_amd import lib
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.encoders import RNNEncoder
    from context_attentive_ir_amd.encoders.rnn_encoder import lstm_cat_weights
    H, M, T_, V, E = 128, 83, 37, 700, 300
    enc = fill_module_(RNNEncoder("LSTM", E, True, 1, 2 * H), seed=9).eval()
    g = torch.Generator().manual_seed(11)
    table = (torch.rand(V, E, generator=g) - 0.5)
    lens = torch.randint(1, T_ + 1, (M,), generator=g); lens[0] = T_; lens[40] = 1
    ids = torch.randint(1, V, (M, T_), generator=g)
    ids[torch.arange(T_)[None] >= lens[:, None]] = 0
    sd = {"e." + k: v for k, v in enc.state_dict().items()}
    _, ref = O.rnn_encode(sd, "e", table[ids], lens)
    wih, whh, bih, bhh = (t.detach().float().contiguous().to(DEV) for t in lstm_cat_weights(enc.rnns[0]))
    folded = lib.fold_lstm_table(table.to(DEV), wih, bih, bhh, H, 2, "f32")
    idd, ld = ids.to(DEV), lens.to(DEV)
    out = torch.full((M, T_, 2 * H), float("nan"), device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.check(lib.load().nir_bilstm_folded_fwd(lib.ptr(folded), lib.DTYPE_F32, lib.ptr(idd), lib.ptr(ld), lib.ptr(whh), lib.ptr(out),
                                               lib.ptr(err), M, V, T_, H, 2, lib.stream()), "folded")
    assert int(err.item()) == 0
    _close(out, ref, 2e-5)


def test_cars_bf16_single_term_attention_pipeline():
    """bf16 encoders hand the attention MLP single fp16 terms in the pipelined kernel (csrc/cars_attn.hip, ONE = true; bench-size
    launches select the pipeline by tile count, here it is forced with attn_unfused_pipe = 2).  The pooled vectors stay within fp16
    rounding of the three-term result (|h| < 1: 2^-11 absolute on the weighted sum, plus the logit perturbation), and the scores stay
    inside the bf16 bound against the fp32 oracle."""
    from context_attentive_ir_amd import lib, synth
    V, B, S, N, QL, DL = 3000, 3, 4, 9, 4, 64
    m = build_model("CARS", vocab=V, device=DEV)
    m.compute_dtype = "bf16"
    ex = synth.session_batch(B, S, N, QL, DL, V, seed=11, full_length=False)
    dex = {k: v.to(DEV) for k, v in ex.items()}
    with lib.tunable("attn_unfused_pipe", 1, 0):
        d3 = m.encode_document(dex["document_words"], dex["document_lens"])
    with lib.tunable("attn_unfused_pipe", 2, 0):
        d1 = m.encode_document(dex["document_words"], dex["document_lens"])
        pooled, _, _ = m.encode(dex["source_words"], dex["source_lens"])
        s, _, _ = m.rank_document(pooled, dex["document_words"], dex["document_lens"], dex["document_labels"])
    assert float((d1 - d3).abs().max()) > 0.0          # the single-term variant really ran
    _close(d1, d3, 2e-3)
    ref = O.cars_scores(cpu_state_dict(m), ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"],
                        ex["document_labels"])
    assert float((s.cpu() - ref).abs().max()) <= BF16_SCORE_TOL
    _close(torch.softmax(s.cpu(), -1), torch.softmax(ref, -1), BF16_PROB_TOL)


def test_cars_bf16_full_c5_shape_against_fp32_path():
    """BASELINE config 5 at its full per-GPU shape (64 sessions x 7 queries x 50 candidates, q_len 4, doc_len 64): here the document
    encoder takes the paths only large launches select -- persistent bf16-table recurrence with fp16 states streamed from LDS, the
    pipelined attention kernel on fp16 rows.  Checked against the fp32 path of the same model on the same batch (itself pinned to
    the oracle at smaller sizes): scores within the bf16 bound, softmax within the probability bound, MAP within BF16_MAP_TOL, and -- size
    independent -- padded candidates / permutation of the candidate axis leave the other scores unchanged."""
    from context_attentive_ir_amd import synth
    from context_attentive_ir_amd.eval import ltorank
    V, B, S, N, QL, DL = 5000, 64, 7, 50, 4, 64
    m = build_model("CARS", vocab=V, device=DEV)
    ex = {k: v.to(DEV) for k, v in synth.session_batch(B, S, N, QL, DL, V, seed=5, full_length=False).items()}

    def scores(model, e):
        pooled, _, _ = model.encode(e["source_words"], e["source_lens"])
        return model.rank_document(pooled, e["document_words"], e["document_lens"], e["document_labels"])[0]

    ref = scores(m, ex).cpu()
    m.compute_dtype = "bf16"
    got = scores(m, ex).cpu()
    assert torch.isfinite(got).all()
    assert float((got - ref).abs().max()) <= BF16_SCORE_TOL, float((got - ref).abs().max())
    _close(torch.softmax(got, -1), torch.softmax(ref, -1), BF16_PROB_TOL)
    lab = ex["document_labels"].reshape(-1, N).cpu().numpy()
    map_ref = ltorank.MAP(np.argsort(-ref.reshape(-1, N).numpy(), 1), lab)
    map_got = ltorank.MAP(np.argsort(-got.reshape(-1, N).numpy(), 1), lab)
    assert abs(map_ref - map_got) <= BF16_MAP_TOL, (map_ref, map_got)
    # permuting the candidates permutes the scores (the click-pooled session state is order independent up to summation order)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1)).to(DEV)
    pex = dict(ex)
    pex["document_words"] = ex["document_words"][:, :, perm]
    pex["document_lens"] = ex["document_lens"][:, :, perm]
    pex["document_labels"] = ex["document_labels"][:, :, perm]
    gp = scores(m, pex).cpu()
    assert float((gp - got[:, :, perm.cpu()]).abs().max()) <= 2e-3


def test_cars_full_c5_shape_against_the_oracle():
    """BASELINE config 5 at its full per-GPU shape (64 sessions x 7 x 50 candidates, d64, ragged lengths) against the ORACLE itself (one CPU pass,
    ~10 s), not against another HIP path: the fp32 path -- the kernels only large launches select: 4.4 rounds of the folded recurrence, the
    attention pipeline on the recurrence's term pairs, B = 64 session steps on the fp16-split kernel -- within 1e-4 on the scores with IDENTICAL
    MAP; the bf16 path within its stated bound, identical ranking on every (session, query) row the oracle separates by more than twice that
    bound, MAP within BF16_MAP_TOL on the rest."""
    from context_attentive_ir_amd import synth
    from context_attentive_ir_amd.eval import ltorank
    V, B, S, N, QL, DL = 5000, 64, 7, 50, 4, 64
    m = build_model("CARS", vocab=V, device=DEV)
    ex = synth.session_batch(B, S, N, QL, DL, V, seed=5, full_length=False)
    ref = O.cars_scores(cpu_state_dict(m), ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"], ex["document_labels"])
    dex = {k: v.to(DEV) for k, v in ex.items()}

    def scores():
        pooled, _, _ = m.encode(dex["source_words"], dex["source_lens"])
        return m.rank_document(pooled, dex["document_words"], dex["document_lens"], dex["document_labels"])[0].cpu()

    lab = ex["document_labels"].reshape(-1, N).numpy()
    r_ref = ref.reshape(-1, N).numpy()
    a_ref = np.argsort(-r_ref, 1, kind="stable")
    got = scores()
    scale = max(1.0, float(ref.abs().max()))
    assert float((got - ref).abs().max()) <= 1e-4 * scale
    a_got = np.argsort(-got.reshape(-1, N).numpy(), 1, kind="stable")
    err = float((got - ref).abs().max())
    sep = np.diff(np.sort(r_ref, 1), axis=1).min(1) > 2.5 * err              # rows whose closest pair of scores is further apart than the error allows to flip
    assert (a_ref[sep] == a_got[sep]).all()
    print("full C5 shape: max |score diff| %.2e (scale %.2f), %d of %d rows separated beyond it" % (err, scale, int(sep.sum()), len(sep)))
    assert abs(ltorank.MAP(a_ref, lab) - ltorank.MAP(a_got, lab)) <= 1e-3
    m.compute_dtype = "bf16"
    got16 = scores()
    assert float((got16 - ref).abs().max()) <= BF16_SCORE_TOL
    _close(torch.softmax(got16, -1), torch.softmax(ref, -1), BF16_PROB_TOL)
    a16 = np.argsort(-got16.reshape(-1, N).numpy(), 1, kind="stable")
    safe = np.diff(np.sort(r_ref, 1), axis=1).min(1) > 2 * BF16_SCORE_TOL
    assert (a_ref[safe] == a16[safe]).all()
    assert abs(ltorank.MAP(a_ref, lab) - ltorank.MAP(a16, lab)) <= BF16_MAP_TOL


def test_cars_split2_precision_tier_vs_oracle():
    """The opt-in 2-MFMA tier (compute_dtype "f32_split2" = NIR_DTYPE_F32_SPLIT2: W_hh two fp16 terms x h ONE fp16 term in the recurrent product,
    fp16 rows into attn_pool_pipe_kernel<false,1>) at a shape where its kernels run (560 documents of 64 tokens): the tier's kernels really ran,
    scores within 1e-4 of the ORACLE at default-scale weights (measured 1.6e-5 against 5.7e-7 of the default path: tools/split2_error_survey.py),
    MAP@10 equal; the default path of the same model is untouched by the switch."""
    import ctypes as C
    from context_attentive_ir_amd import lib, synth
    from context_attentive_ir_amd.eval import ltorank
    V, B, S, N, QL, DL = 20000, 8, 7, 10, 4, 64
    m = build_model("CARS", vocab=V, device=DEV)
    ex = synth.session_batch(B, S, N, QL, DL, V, seed=3, full_length=True)
    ref = O.cars_scores(cpu_state_dict(m), ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"], ex["document_labels"])
    dex = {k: v.to(DEV) for k, v in ex.items()}

    def run():
        pooled, _, _ = m.encode(dex["source_words"], dex["source_lens"])
        return m.rank_document(pooled, dex["document_words"], dex["document_lens"], dex["document_labels"], want_states=False)[0]
    base = run().cpu()
    m.compute_dtype = "f32_split2"
    L = lib.load()
    L.nir_profile_enable(1)
    got = run().cpu()
    torch.cuda.synchronize()
    L.nir_profile_enable(0)
    buf = C.create_string_buffer(1 << 16)
    L.nir_profile_report(buf, len(buf))
    names = {ln.rsplit(",", 2)[0].split("[")[0] for ln in buf.value.decode().strip().splitlines()}
    assert "lstm16_pt_h2_kernel<4,4,8,true>" in names and "attn_pool_pipe_kernel<false,1>" in names, names
    err = float((got - ref).abs().max())
    assert 1e-6 < err <= 1e-4, err                                   # (not the parity path: its error is visible, and inside the bar)
    assert float((base - ref).abs().max()) <= 2e-6
    lab = ex["document_labels"].reshape(-1, N).numpy().astype(int)
    a_ref, a_got = (np.argsort(-t.reshape(-1, N).numpy(), 1, kind="stable") for t in (ref, got))
    assert ltorank.MAP(a_ref, lab) == ltorank.MAP(a_got, lab)
    m.compute_dtype = "f32"
    assert torch.equal(run().cpu(), base)
