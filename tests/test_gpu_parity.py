"""GPU (-m gpu): the HIP path, called through the C-ABI, against (a) the committed golden vectors from the real
reference and (b) the CPU oracle on seeded synthetic inputs.  Tolerance: 1e-4 absolute on fp32 scores
(BASELINE.json north_star); integer histogram counts are compared exactly on edge-safe inputs."""
import os

import numpy as np
import pytest
import torch

from conftest import T, load_golden
from helpers import build_model, cpu_state_dict
from oracle import neuroir_cpu as O

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda"


def _close(a, b, tol=TOL):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=0, atol=tol)


def _synth(rng, B, N, QL, DL, V, full=False):
    qlen = rng.integers(1, QL + 1, size=B); dlen = rng.integers(1, DL + 1, size=(B, N))
    if full:
        qlen[:] = QL; dlen[:] = DL
    qlen[0] = QL; dlen[0, 0] = DL
    q = rng.integers(4, V, size=(B, QL)); d = rng.integers(4, V, size=(B, N, DL))
    q[np.arange(QL)[None] >= qlen[:, None]] = 0
    d[np.arange(DL)[None, None] >= dlen[..., None]] = 0
    return [torch.from_numpy(x.astype(np.int64)) for x in (q, qlen, d, dlen)]


# ------------------------------------------------------------------ building blocks
@pytest.mark.parametrize("M,N,K,act", [(37, 40, 300, 0), (130, 50, 30, 0), (64, 64, 32, 1), (257, 301, 900, 2), (5, 1, 7, 0),
                                       (16, 2048, 768, 0), (1100, 800, 260, 1), (20480, 40, 300, 0), (3000, 70, 35, 2),
                                       (8200, 512, 301, 1), (4100, 1024, 70, 2), (33000, 128, 64, 0),
                                       (5000, 50, 140, 0), (4100, 64, 300, 1), (4097, 17, 20, 2), (20481, 33, 8, 0),
                                       # large enough for the split-precision (3 x bf16) kernel: ragged M/N/K tails included
                                       (13000, 300, 900, 1), (71680, 256, 256, 0), (12289, 129, 36, 2), (40000, 1024, 300, 0),
                                       # mid-size: the 32x32-block exact-fp32 kernel (CARS maxout shapes; ragged M / N tails)
                                       (1120, 512, 1024, 0), (1101, 250, 256, 1), (999, 300, 64, 2),
                                       # small grids of the split-precision kernel (96 .. 511 tiles of 128 x 128): KS k-tiles per pipeline stage, ragged
                                       # M / N tails, K not a multiple of the stage (136 = 2 x 64 + 8), K = one stage + tail
                                       (896, 2048, 256, 0), (8960, 256, 256, 1), (1500, 1100, 136, 2), (8960, 512, 1024, 0), (2000, 900, 132, 0)])
def test_linear_dense(M, N, K, act):
    from context_attentive_ir_amd import lib
    g = torch.Generator().manual_seed(M * 1000 + N)
    a = torch.randn(M, K, generator=g); w = torch.randn(N, K, generator=g) / K ** 0.5; b = torch.randn(N, generator=g)
    ref = torch.nn.functional.linear(a, w, b)
    ref = torch.tanh(ref) if act == 1 else torch.relu(ref) if act == 2 else ref
    ad, wd, bd = a.to(DEV), w.to(DEV), b.to(DEV)
    c = torch.empty(M, N, device=DEV)
    lib.check(lib.load().nir_linear_f32(lib.ptr(ad), K, None, None, 0, 0, 0, lib.ptr(wd), K, lib.ptr(bd), None,
                                        lib.ptr(c), N, M, N, K, act, lib.stream()), "linear")
    _close(c, ref, 2e-5)


def test_linear_gather_conv():
    """Conv1d(E->F, k=3) over gathered embeddings == the GEMM with K=3E and the [F][3][E] weight layout."""
    from context_attentive_ir_amd import lib
    g = torch.Generator().manual_seed(7)
    V, E, F_, nseq, L = 50, 300, 70, 5, 11
    _gather_conv_case(lib, g, V, E, F_, nseq, L)
    _gather_conv_case(lib, g, 500, 300, 300, 400, 40)       # large enough for the 64x64-tile kernel
    _gather_conv_case(lib, g, 500, 300, 256, 900, 40)       # N % 128 == 0 and >= 256 tiles: the 128x128-tile kernel
    _gather_conv_case(lib, g, 3000, 300, 300, 450, 64)      # DUET conv shape: split-precision kernel, 3 taps, N tail


@pytest.mark.parametrize("world,B,per,N", [(8, 32, 10, 80), (8, 64, 7, 50), (2, 3, 1, 2), (1, 5, 130, 130), (4, 1, 40, 157)])
def test_softmax_gathered(world, B, per, N):
    """softmax straight off the rank-major all-gather buffer == softmax of the re-assembled [B,N] score rows."""
    from context_attentive_ir_amd import lib
    g = torch.Generator().manual_seed(world * 100 + N)
    gathered = torch.randn(world, B, per, generator=g) * 3
    full = gathered.permute(1, 0, 2).reshape(B, world * per)[:, :N]
    gd = gathered.to(DEV)
    probs = torch.empty(B, N, device=DEV); raw = torch.empty(B, N, device=DEV)
    lib.check(lib.load().nir_softmax_gathered(lib.ptr(gd), lib.ptr(probs), lib.ptr(raw), world, B, per, N, lib.stream()), "sg")
    assert torch.equal(raw.cpu(), full)
    _close(probs, torch.softmax(full, -1), 1e-6)


def test_linear_gather_skinny():
    """Embedding gather + Linear(E -> N <= 64) over many token rows: the LDS-resident-W skinny kernel (PAD row stays zero)."""
    from context_attentive_ir_amd import lib
    g = torch.Generator().manual_seed(11)
    for V, E, N, M in ((300, 300, 40, 20608), (50, 64, 64, 4099), (1000, 300, 7, 9000)):
        table = torch.randn(V, E, generator=g); table[0] = 0
        ids = torch.randint(0, V, (M,), generator=g)
        w = torch.randn(N, E, generator=g) / E ** 0.5; b = torch.randn(N, generator=g)
        ref = torch.tanh(table[ids] @ w.t() + b)
        idd, td, wd, bd = ids.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV)
        out = torch.empty(M, N, device=DEV)
        lib.check(lib.load().nir_linear_f32(None, 0, lib.ptr(idd), lib.ptr(td), E, 1, 1, lib.ptr(wd), E, lib.ptr(bd), None,
                                            lib.ptr(out), N, M, N, E, 1, lib.stream()), "linear")
        _close(out, ref, 2e-5)


def _gather_conv_case(lib, g, V, E, F_, nseq, L):
    table = torch.randn(V, E, generator=g); ids = torch.randint(0, V, (nseq, L), generator=g)
    w = torch.randn(F_, E, 3, generator=g) / 30; b = torch.randn(F_, generator=g)
    ref = torch.nn.functional.conv1d(table[ids].transpose(1, 2), w, b).transpose(1, 2)   # [nseq, L-2, F]
    wd = w.permute(0, 2, 1).contiguous().to(DEV)
    idd, td, bd = ids.to(DEV), table.to(DEV), b.to(DEV)       # keep device copies alive across the async launch
    out = torch.empty(nseq * (L - 2), F_, device=DEV)
    lib.check(lib.load().nir_linear_f32(None, 0, lib.ptr(idd), lib.ptr(td), E, L - 2, L, lib.ptr(wd), 3 * E,
                                        lib.ptr(bd), None, lib.ptr(out), F_, nseq * (L - 2), F_, 3 * E, 0,
                                        lib.stream()), "linear")
    _close(out.view(nseq, L - 2, F_), ref, 2e-5)


@pytest.mark.parametrize("H,I,M,T_", [(15, 40, 7, 6), (70, 40, 33, 20), (128, 300, 19, 12), (128, 300, 700, 9), (32, 16, 1200, 5),
                                      (70, 100, 21, 17), (40, 100, 9, 30), (96, 64, 5, 8), (1, 1, 3, 4)])
def test_rnn_encoder(H, I, M, T_):
    from context_attentive_ir_amd.encoders import RNNEncoder
    from context_attentive_ir_amd.detinit import fill_module_
    enc = fill_module_(RNNEncoder("LSTM", I, True, 1, 2 * H), seed=3).eval()
    g = torch.Generator().manual_seed(H + M)
    x = torch.randn(M, T_, I, generator=g); lens = torch.randint(1, T_ + 1, (M,), generator=g); lens[0] = T_
    sd = {"e." + k: v for k, v in enc.state_dict().items()}
    (hn_ref, cn_ref), ref = O.rnn_encode(sd, "e", x, lens)
    enc = enc.to(DEV)
    (hn, cn), out = enc(x.to(DEV), lens.to(DEV))
    # 5e-6: the recurrence alone is held to <= 3.6e-6 against float64 at such shapes (tests/test_gpu_rnn_envelope.py), this oracle is an fp32
    # chain itself (<= 6e-7) and the input GEMM over I = 300 adds ~1e-6 to the gates; measured worst 1.9e-6 (H = 128, I = 300, 1100 sequences)
    _close(out, ref, 5e-6)
    order = torch.sort(lens, 0, True)[1]                   # reference leaves final states in sorted order
    _close(hn[:, order], hn_ref, 5e-6); _close(cn[:, order], cn_ref, 5e-6)


@pytest.mark.parametrize("H,I,M,T_", [(70, 40, 37, 20), (15, 40, 50, 6), (128, 300, 40, 12), (96, 64, 21, 8), (96, 100, 33, 9),
                                      (40, 16, 17, 11), (128, 24, 19, 7)])
def test_rnn_encoder_16_sequence_layout(H, I, M, T_, monkeypatch):
    """The 16-sequence 16x16x4-MFMA recurrences (chosen by the library only from ~1000 sequences up) forced on small,
    ragged batches: partial workgroups, one- and two-tile waves, fused and unfused input projection."""
    from context_attentive_ir_amd import lib
    with lib.tunable("lstm_mfma16", 1, restore=-1):
        test_rnn_encoder(H, I, M, T_)


def test_rnn_encoder_many_sequences():
    """Enough sequences for the library to pick the 16-sequence layouts on its own (fused H=70/I=40, unfused H=128/I=300)."""
    test_rnn_encoder(70, 40, 1300, 5)
    test_rnn_encoder(128, 300, 1100, 4)


def test_losses_softmax_golden():
    from context_attentive_ir_amd import lib
    g = load_golden("losses_metrics")
    s, y = T(g["scores"], DEV), T(g["labels"], DEV).float()
    L = lib.load()
    out = torch.empty_like(s); loss = torch.empty(2, device=DEV)
    lib.check(L.nir_softmax_rows(lib.ptr(s), lib.ptr(out), s.shape[0], s.shape[1], lib.stream()), "softmax")
    lib.check(L.nir_rank_loss_bce(lib.ptr(s), lib.ptr(y), s.shape[0], s.shape[1], lib.ptr(loss), lib.stream()), "bce")
    lib.check(L.nir_rank_loss_softmax_nll(lib.ptr(s), lib.ptr(y), s.shape[0], s.shape[1], C_off(loss, 1), lib.stream()), "nll")
    _close(out, g["softmax"], 1e-6); _close(loss[0], g["bce"], 1e-6); _close(loss[1], g["softmax_nll"], 1e-6)


def C_off(t, i):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + 4 * i)


# ------------------------------------------------------------------ ESM
def test_esm_golden():
    g = load_golden("esm")
    m = build_model("ESM", device=DEV)
    s = m(T(g["que_rep"], DEV), T(g["que_len"], DEV), T(g["doc_rep"], DEV), T(g["doc_len"], DEV))
    _close(s, g["scores"])
    assert s[1, 2].item() == 0.0


@pytest.mark.parametrize("B,N,QL,DL", [(8, 5, 4, 64), (3, 50, 6, 290), (1, 1, 1, 1), (2, 7, 20, 130)])
def test_esm_oracle(B, N, QL, DL):
    rng = np.random.default_rng(B * 100 + N)
    m = build_model("ESM", vocab=5000, device=DEV)
    q, ql, d, dl = _synth(rng, B, N, QL, DL, 5000)
    ref = O.esm_scores(cpu_state_dict(m), q, ql, d, dl)
    _close(m(q.to(DEV), ql.to(DEV), d.to(DEV), dl.to(DEV)), ref)


# ------------------------------------------------------------------ MatchTensor
def test_match_tensor_golden():
    g = load_golden("match_tensor")
    m = build_model("MATCH_TENSOR", device=DEV)
    s, (hq, hd, pq, pd) = m(T(g["que_rep"], DEV), T(g["que_len"], DEV), T(g["doc_rep"], DEV), T(g["doc_len"], DEV),
                            return_parts=True)
    _close(hq, g["enc_q"], 2e-5); _close(hd, g["enc_d"], 2e-5)
    _close(pq, g["proj_q"], 2e-5); _close(pd, g["proj_d"], 2e-5)
    _close(s, g["scores"])


@pytest.mark.parametrize("B,N,QL,DL,full", [(32, 10, 4, 64, True), (4, 3, 6, 64, False), (2, 5, 1, 7, False), (3, 2, 9, 130, False),
                                            (2, 3, 6, 290, True), (3, 50, 4, 290, False)])      # max_doc_len recurrences (T = 290)
def test_match_tensor_oracle(B, N, QL, DL, full):
    rng = np.random.default_rng(B * 100 + DL)
    m = build_model("MATCH_TENSOR", vocab=300, device=DEV)     # small vocab -> exact-match channel is exercised
    q, ql, d, dl = _synth(rng, B, N, QL, DL, 300, full)
    ref = O.match_tensor_scores(cpu_state_dict(m), q, ql, d, dl)
    _close(m(q.to(DEV), ql.to(DEV), d.to(DEV), dl.to(DEV)), ref)


# ------------------------------------------------------------------ DRMM
def test_drmm_golden_safe():
    g = load_golden("drmm_safe")
    m = build_model("DRMM", device=DEV)
    s, hist = m(T(g["que_rep"], DEV), T(g["que_len"], DEV), T(g["doc_rep"], DEV), T(g["doc_len"], DEV), return_hist=True)
    np.testing.assert_array_equal(hist.cpu().numpy(), g["hist"].astype(np.float32))
    _close(s, g["scores"])


def test_drmm_golden_overlap_exact():
    """Appendix E1 closed (round 5): at an exact token overlap the reference's cosine of the row with itself is <1 / ==1 / >1 by ITS reduction
    order; that bin is a function of the embedding row, looked up by the kernel (exact_match_policy 'reference', the default) -- the
    integer histograms of the real reference's overlap fixture are reproduced EXACTLY, and with them the scores."""
    g = load_golden("drmm_overlap")
    m = build_model("DRMM", device=DEV)
    assert m.exact_match_policy == "reference"
    s, hist = m(T(g["que_rep"], DEV), T(g["que_len"], DEV), T(g["doc_rep"], DEV), T(g["doc_len"], DEV), return_hist=True)
    q, d = g["que_rep"], g["doc_rep"]
    assert int(((q[:, None, :, None] == d[:, :, None, :]) & (q[:, None, :, None] != 0)).sum()) > 0
    np.testing.assert_array_equal(hist.cpu().numpy(), g["hist"].astype(np.float32))
    _close(s, g["scores"])


def test_drmm_golden_overlap_policy():
    """The kernel's OWN cosine at exact overlaps (policy 'numpy', rounds 1-4): 1 +- 1 ulp depending on the reduction order, so numpy.histogram
    puts it into [.5,1), {1} or drops it.  What IS pinned there: (a) the three lower bins
    never differ from the reference, (b) a (pair, query term) row can only differ in the two top bins, by at most 2 per exact
    overlap of that query term (one count leaving a bin, one entering another), (c) pairs whose histograms agree agree in score,
    (d) the number of affected pairs on the fixture is the measured 6 of 12 (+-1: one overlap sits exactly on the rounding edge)."""
    g = load_golden("drmm_overlap")
    m = build_model("DRMM", device=DEV)
    m.exact_match_policy = "numpy"
    s, hist = m(T(g["que_rep"], DEV), T(g["que_len"], DEV), T(g["doc_rep"], DEV), T(g["doc_len"], DEV), return_hist=True)
    h, r = hist.cpu().numpy(), g["hist"]
    q, d = g["que_rep"], g["doc_rep"]
    B, N, DL = d.shape
    np.testing.assert_array_equal(h[..., :3], r[..., :3])                                                   # (a)
    overlaps = ((q[:, None, :, None] == d[:, :, None, :]) & (q[:, None, :, None] != 0)).sum(-1)              # [B,N,QL]
    top_diff = np.abs(h[..., 3:] - r[..., 3:]).sum(-1).reshape(B, N, -1)
    assert (top_diff <= 2 * overlaps).all()                                                                  # (b)
    same = (h == r).all(axis=(1, 2))
    _close(s.cpu().numpy().reshape(-1)[same], g["scores"].reshape(-1)[same])                                 # (c)
    assert abs(int((~same).sum()) - 6) <= 1, int((~same).sum())                                              # (d)
    assert (h.sum(-1) <= DL).all()


@pytest.mark.parametrize("B,N,QL,DL", [(4, 6, 4, 290), (2, 3, 12, 64)])
def test_drmm_oracle(B, N, QL, DL):
    rng = np.random.default_rng(QL)
    V = 5000
    m = build_model("DRMM", vocab=V, device=DEV)
    q, ql, d, dl = _synth(rng, B, N, QL, DL, V)
    q[q > 0] = q[q > 0] % 1000 + 4; d[d > 0] = d[d > 0] % 3000 + 1500      # disjoint vocab halves: edge-safe
    sd = cpu_state_dict(m)
    gate, cos, hist_ref = O.drmm_parts(sd, q, d)
    s, hist = m(q.to(DEV), ql.to(DEV), d.to(DEV), dl.to(DEV), return_hist=True)
    c = cos.numpy(); edge = np.abs(c[..., None] - np.array([-1, -.5, 0, .5, 1.0])).min(-1); edge[c == 0] = 1
    safe = (edge > 2e-6).all(axis=(1, 2))
    np.testing.assert_array_equal(hist.cpu().numpy()[safe], hist_ref.numpy()[safe])
    ref = O.drmm_scores_from_hist(sd, gate, hist_ref, B, N).reshape(-1)
    _close(s.reshape(-1)[torch.from_numpy(safe)], ref[torch.from_numpy(safe)], 2e-4)   # |scores| ~ 20 -> relative 1e-5


# ------------------------------------------------------------------ DUET
def test_duet_golden():
    g = load_golden("duet")
    QL, DL = g["que_rep"].shape[1], g["doc_rep"].shape[2]
    m = build_model("DUET", device=DEV, max_query_len=QL, max_doc_len=DL)
    s, loc, dist = m(T(g["que_rep"], DEV), T(g["que_len"], DEV), T(g["doc_rep"], DEV), T(g["doc_len"], DEV), return_parts=True)
    _close(loc, g["local"]); _close(dist, g["dist"]); _close(s, g["scores"])


@pytest.mark.parametrize("B,N,QL,DL", [(3, 4, 4, 64), (2, 3, 6, 290), (1, 2, 3, 7)])
def test_duet_oracle(B, N, QL, DL):
    rng = np.random.default_rng(DL)
    m = build_model("DUET", vocab=400, device=DEV, max_query_len=QL, max_doc_len=DL)
    q, ql, d, dl = _synth(rng, B, N, QL, DL, 400)
    sd = cpu_state_dict(m)
    s, loc, dist = m(q.to(DEV), ql.to(DEV), d.to(DEV), dl.to(DEV), return_parts=True)
    _close(loc, O.duet_local(sd, q, d)); _close(dist, O.duet_distributed(sd, q, d))
    _close(s, O.duet_scores(sd, q, ql, d, dl))


def test_duet_rejects_unpadded_and_short_query():
    m = build_model("DUET", device=DEV, max_query_len=5, max_doc_len=24)
    q = torch.zeros(2, 4, dtype=torch.long, device=DEV); d = torch.zeros(2, 3, 24, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError):
        m(q, None, d, None)
    m2 = build_model("DUET", device=DEV, max_query_len=2, max_doc_len=24)
    with pytest.raises(RuntimeError):   # QL < 3: the reference's Conv1d(k=3) is invalid too
        m2(torch.zeros(2, 2, dtype=torch.long, device=DEV), None, d, None)


# ------------------------------------------------------------------ CARS
@pytest.mark.parametrize("tag", ["oneclick", "multiclick"])
def test_cars_golden(tag):
    g = load_golden("cars_" + tag)
    m = build_model("CARS", device=DEV)
    q, ql, d, dl, lab = (T(g[k], DEV) for k in ("source_words", "source_lens", "document_words", "document_lens", "document_labels"))
    pooled, enc, _ = m.encode(q, ql)
    _close(enc, g["enc_q"], 2e-5); _close(pooled, g["pooled_q"], 2e-5)
    docs = m.encode_document(d, dl)
    _close(docs, g["pooled_docs"], 2e-5)
    _close(m.encode_clicks(docs, lab), g["encoded_clicks"], 2e-5)
    scores, _, _ = m.rank_document(pooled, d, dl, lab)
    _close(scores, g["click_scores"])
    out = m(q, ql, None, None, None, d, dl, lab)
    _close(out["ranking_loss"], g["ranking_loss"], 1e-5)


@pytest.mark.parametrize("B,S,N,QL,DL,multi", [(16, 7, 10, 4, 64, False), (3, 2, 50, 6, 33, True), (2, 1, 1, 3, 5, False),
                                               (2, 2, 5, 40, 290, True)])                       # max_doc_len / max query length recurrences
def test_cars_oracle(B, S, N, QL, DL, multi):
    from context_attentive_ir_amd import synth
    V = 3000
    m = build_model("CARS", vocab=V, device=DEV)
    ex = synth.session_batch(B, S, N, QL, DL, V, seed=B * 10 + S, full_length=False, multi_click=multi)
    sd = cpu_state_dict(m)
    ref = O.cars_scores(sd, ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"], ex["document_labels"])
    dex = {k: v.to(DEV) for k, v in ex.items()}
    pooled, _, _ = m.encode(dex["source_words"], dex["source_lens"])
    s, _, _ = m.rank_document(pooled, dex["document_words"], dex["document_lens"], dex["document_labels"])
    _close(s, ref)


# ------------------------------------------------------------------ wrappers / MAP parity
def test_ranker_predict_and_map_parity():
    """MAP@10 parity through the Ranker wrapper (predict = softmax(network(...))).  DRMM runs on OVERLAPPING ids (queries and documents
    share tokens: the exact-match bins carry signal) since round 5 -- the self-cosine bin table reproduces the reference's histogram there."""
    from context_attentive_ir_amd import synth
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.eval import MAP, rank_candidates
    from context_attentive_ir_amd.wrappers import Ranker
    V = 3000
    for kind in ("ESM", "MATCH_TENSOR", "DRMM", "DUET"):
        ex = synth.ranker_batch(16, 10, 4, 64, V, seed=5, full_length=(kind == "DUET"))
        if kind == "DRMM":
            q, d = ex["que_rep"], ex["doc_rep"]
            q[q > 0] = q[q > 0] % 400 + 4                       # a 400-word vocabulary: every candidate shares tokens with its query
            d[d > 0] = d[d > 0] % 400 + 4
            assert int(((q[:, None, :, None] == d[:, :, None, :]) & (q[:, None, :, None] != 0)).sum()) > 200
        extra = dict(max_query_len=4, max_doc_len=64) if kind == "DUET" else {}
        r = Ranker(default_args(kind, src_vocab_size=V, **extra)); fill_module_(r.network, 1013); r.cuda()
        got = r.predict(ex).cpu()
        sd = {k: v.detach().cpu() for k, v in r.network.state_dict().items()}
        ref = O.predict_softmax(O.MODEL_FNS[kind](sd, ex["que_rep"], ex["que_len"], ex["doc_rep"], ex["doc_len"]))
        _close(got, ref)
        assert MAP(rank_candidates(got.numpy()), ex["label"].numpy()) == pytest.approx(
            O.mean_average_precision(rank_candidates(ref.numpy()), ex["label"].numpy()), abs=1e-12), kind


def test_drmm_map_on_overlapping_zipf_ids_is_bounded():
    """DRMM where its exact-match signal lives (Zipf ids: queries and documents share tokens).  The top two histogram bins are not reproducible
    at an exact overlap (cos = 1 +- 1 ulp), so MAP is not asserted equal but BOUNDED: |MAP_hip - MAP_oracle| <= 0.03 for
    both exact-match policies on a 16 x 50 x 290 slice (measured: +0.0117 default, -0.0015 'snap'; random-weight model, the worst case for
    near-ties), and the predict softmax agrees with the oracle on every pair whose histogram does."""
    from context_attentive_ir_amd import synth
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.eval import MAP, rank_candidates
    from context_attentive_ir_amd.wrappers import Ranker
    V, B, N, QL, DL = 100000, 16, 50, 4, 290
    ex = synth.ranker_batch(B, N, QL, DL, V, seed=1013, full_length=False)
    r = Ranker(default_args("DRMM", src_vocab_size=V)); fill_module_(r.network, 1013); r.cuda()
    sd = {k: v.detach().cpu() for k, v in r.network.state_dict().items()}
    gate, _, hist_ref = O.drmm_parts(sd, ex["que_rep"], ex["doc_rep"])
    s_ref = O.drmm_scores_from_hist(sd, gate, hist_ref, B, N)
    ref = O.predict_softmax(s_ref)
    map_ref = MAP(rank_candidates(ref.numpy()), ex["label"].numpy())
    overlaps = int(((ex["que_rep"][:, None, :, None] == ex["doc_rep"][:, :, None, :]) & (ex["que_rep"][:, None, :, None] != 0)).sum())
    assert overlaps > 50
    for policy in ("reference", "numpy", "snap"):
        r.network.exact_match_policy = policy
        got = r.predict(ex).cpu()
        assert abs(MAP(rank_candidates(got.numpy()), ex["label"].numpy()) - map_ref) <= 0.03, policy
        _, h = r.network(ex["que_rep"].cuda(), ex["que_len"].cuda(), ex["doc_rep"].cuda(), ex["doc_len"].cuda(), return_hist=True)
        same = (h.cpu().numpy() == hist_ref.numpy()).all(axis=(1, 2)).reshape(B, N)
        if policy == "reference":      # the default: histograms are the reference's (<= 5 of 3 200 rows may sit on a true rounding edge between DIFFERENT rows)
            rows_differ = int((h.cpu().numpy() != hist_ref.numpy()).any(axis=2).sum())
            assert rows_differ <= 5, rows_differ
            if rows_differ == 0:
                _close(got, ref)
                assert MAP(rank_candidates(got.numpy()), ex["label"].numpy()) == map_ref
        rows = same.all(1)                                      # queries all of whose candidates have the oracle's histogram: softmax must agree
        if rows.any():
            _close(got[rows], ref[rows])


def test_multitask_predict_map_parity():
    from context_attentive_ir_amd import synth
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.eval import MAP, rank_candidates
    from context_attentive_ir_amd.wrappers import Multitask
    V = 3000
    ex = synth.session_batch(4, 5, 10, 4, 48, V, seed=11, full_length=False)
    mt = Multitask(default_args("CARS", src_vocab_size=V)); fill_module_(mt.network, 1013); mt.cuda()
    got = mt.predict(ex)["click_scores"].cpu()
    sd = {k: v.detach().cpu() for k, v in mt.network.state_dict().items()}
    ref = O.predict_softmax(O.cars_scores(sd, ex["source_words"], ex["source_lens"], ex["document_words"],
                                          ex["document_lens"], ex["document_labels"]))
    _close(got, ref)
    lab = ex["document_labels"].numpy().reshape(-1, 10).astype(np.int64)
    assert MAP(rank_candidates(got.numpy().reshape(-1, 10)), lab) == pytest.approx(
        O.mean_average_precision(rank_candidates(ref.numpy().reshape(-1, 10)), lab), abs=1e-12)


# ------------------------------------------------------------------ properties
@pytest.mark.parametrize("kind", ["ESM", "MATCH_TENSOR", "DRMM", "DUET"])
def test_candidate_permutation_permutes_scores(kind):
    """Every (query, candidate) pair is independent given the query: permuting candidates permutes scores."""
    rng = np.random.default_rng(17)
    B, N, QL, DL, V = 3, 7, 4, 24, 500
    extra = dict(max_query_len=QL, max_doc_len=DL) if kind == "DUET" else {}
    m = build_model(kind, vocab=V, device=DEV, **extra)
    q, ql, d, dl = (t.to(DEV) for t in _synth(rng, B, N, QL, DL, V, full=(kind == "DUET")))
    perm = torch.from_numpy(rng.permutation(N)).to(DEV)
    s0 = m(q, ql, d, dl)
    s1 = m(q, ql, d[:, perm].contiguous(), dl[:, perm].contiguous())
    _close(s1, s0[:, perm], 1e-6)


def test_empty_batch_and_single_token():
    m = build_model("ESM", device=DEV)
    q = torch.zeros(0, 4, dtype=torch.long, device=DEV); d = torch.zeros(0, 3, 8, dtype=torch.long, device=DEV)
    assert m(q, q[:, 0], d, d[:, :, 0]).shape == (0, 3)
    mt = build_model("MATCH_TENSOR", device=DEV)
    q1 = torch.full((1, 1), 5, dtype=torch.long, device=DEV); d1 = torch.full((1, 1, 1), 5, dtype=torch.long, device=DEV)
    one = torch.ones(1, dtype=torch.long, device=DEV)
    ref = O.match_tensor_scores(cpu_state_dict(mt), q1.cpu(), one.cpu(), d1.cpu(), one.cpu().view(1, 1))
    _close(mt(q1, one, d1, one.view(1, 1)), ref)


def test_graphed_predictor_matches_eager():
    from context_attentive_ir_amd import synth
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.graph_runner import GraphedPredictor
    from context_attentive_ir_amd.wrappers import Ranker
    V = 2000
    r = Ranker(default_args("MATCH_TENSOR", src_vocab_size=V)); fill_module_(r.network, 1013); r.cuda()
    exs = [synth.ranker_batch(8, 6, 4, 32, V, seed=s, full_length=False) for s in (1, 2, 3)]
    gp = GraphedPredictor(r, {k: v.cuda() for k, v in exs[0].items()})
    for ex in exs:                                    # host (unpinned or pinned) ids -> static buffers -> replay
        eager = r.predict(ex)
        _close(gp.predict({k: v.pin_memory() for k, v in ex.items()}), eager, 1e-7)
    with pytest.raises(RuntimeError):
        gp.predict(synth.ranker_batch(4, 6, 4, 32, V))


# ------------------------------------------------------------------ randomized shapes vs the oracle
def _fuzz_shapes(seed, n, ql_max, dl_max, n_max=12, b_max=5):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(1, b_max + 1)), int(rng.integers(1, n_max + 1)), int(rng.integers(1, ql_max + 1)),
             int(rng.integers(1, dl_max + 1))) for _ in range(n)]


@pytest.mark.parametrize("B,N,QL,DL", _fuzz_shapes(101, 8, 20, 150))
def test_fuzz_esm_match_tensor(B, N, QL, DL):
    rng = np.random.default_rng(B * 1000 + DL)
    V = 400
    q, ql, d, dl = _synth(rng, B, N, QL, DL, V)
    for kind, fn in (("ESM", O.esm_scores), ("MATCH_TENSOR", O.match_tensor_scores)):
        m = build_model(kind, vocab=V, device=DEV)
        _close(m(q.to(DEV), ql.to(DEV), d.to(DEV), dl.to(DEV)), fn(cpu_state_dict(m), q, ql, d, dl))


@pytest.mark.parametrize("B,N,QL,DL", [(b, n, max(q, 3), max(d, 7)) for b, n, q, d in _fuzz_shapes(202, 6, 12, 120)])
def test_fuzz_duet(B, N, QL, DL):
    rng = np.random.default_rng(QL * 1000 + DL)
    V = 300
    m = build_model("DUET", vocab=V, device=DEV, max_query_len=QL, max_doc_len=DL)
    q, ql, d, dl = _synth(rng, B, N, QL, DL, V)
    _close(m(q.to(DEV), ql.to(DEV), d.to(DEV), dl.to(DEV)), O.duet_scores(cpu_state_dict(m), q, ql, d, dl))


@pytest.mark.parametrize("B,N,QL,DL", _fuzz_shapes(303, 6, 20, 200))
def test_fuzz_drmm_histograms(B, N, QL, DL):
    rng = np.random.default_rng(N * 1000 + DL)
    V = 6000
    m = build_model("DRMM", vocab=V, device=DEV)
    q, ql, d, dl = _synth(rng, B, N, QL, DL, V)
    q[q > 0] = q[q > 0] % 1000 + 4; d[d > 0] = d[d > 0] % 3000 + 2000          # edge-safe: disjoint vocab halves
    sd = cpu_state_dict(m)
    gate, cos, hist_ref = O.drmm_parts(sd, q, d)
    s, hist = m(q.to(DEV), ql.to(DEV), d.to(DEV), dl.to(DEV), return_hist=True)
    c = cos.numpy(); edge = np.abs(c[..., None] - np.array([-1, -.5, 0, .5, 1.0])).min(-1); edge[c == 0] = 1
    safe = (edge > 2e-6).all(axis=(1, 2))
    np.testing.assert_array_equal(hist.cpu().numpy()[safe], hist_ref.numpy()[safe])
    ref = O.drmm_scores_from_hist(sd, gate, hist_ref, B, N).reshape(-1)
    _close(s.reshape(-1)[torch.from_numpy(safe)], ref[torch.from_numpy(safe)], 5e-4)   # |scores| up to ~1e2


@pytest.mark.parametrize("B,S,N,QL,DL", [(2, 4, 7, 9, 41), (1, 9, 3, 2, 17), (3, 2, 12, 20, 80), (2, 5, 64, 3, 9)])
def test_fuzz_cars(B, S, N, QL, DL):
    from context_attentive_ir_amd import synth
    V = 1500
    m = build_model("CARS", vocab=V, device=DEV)
    ex = synth.session_batch(B, S, N, QL, DL, V, seed=B * 7 + S, full_length=False, multi_click=True)
    ref = O.cars_scores(cpu_state_dict(m), ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"],
                        ex["document_labels"])
    dex = {k: v.to(DEV) for k, v in ex.items()}
    pooled, _, _ = m.encode(dex["source_words"], dex["source_lens"])
    s, _, _ = m.rank_document(pooled, dex["document_words"], dex["document_lens"], dex["document_labels"])
    _close(s, ref)


def test_parallel_predict_one_rank_rccl():
    """Ranker.parallelize(): candidate sharding + RCCL all-gather + nir_softmax_gathered, on a 1-rank 'nccl' group, must
    reproduce the unsharded predict exactly (the N>1 arithmetic is covered by the 2-rank gloo tests on CPU)."""
    import torch.distributed as dist
    from context_attentive_ir_amd.wrappers import Ranker
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29571")
    started = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV, 0))
        started = True
    try:
        w = Ranker(default_args("MATCH_TENSOR", src_vocab_size=300))
        fill_module_(w.network, 5)
        w.cuda()
        q, ql, d, dl = _synth(np.random.default_rng(3), 4, 7, 5, 33, 300)
        ex = {"que_rep": q, "que_len": ql, "doc_rep": d, "doc_len": dl}
        ref, ref_scores = w.predict(ex), w.scores(ex)
        w.parallelize()
        assert torch.equal(w.predict(ex).cpu(), ref.cpu())
        assert torch.equal(w.scores(ex).cpu(), ref_scores.cpu())
    finally:
        if started:
            dist.destroy_process_group()


def test_batchify_to_graphed_predictor():
    """inputters.ranker_batchify -> one packed (pinned) buffer -> GraphedPredictor's single-copy fast path == eager predict."""
    from context_attentive_ir_amd.inputters import ranker_batchify, flat_examples
    from context_attentive_ir_amd.graph_runner import GraphedPredictor
    from context_attentive_ir_amd.wrappers import Ranker
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    w = Ranker(default_args("MATCH_TENSOR", src_vocab_size=300))
    fill_module_(w.network, 9)
    w.cuda()
    rng = np.random.default_rng(21)

    def make(seed):
        r = np.random.default_rng(seed)
        B, N = 6, 5
        q = [r.integers(4, 300, size=r.integers(1, 6)) for _ in range(B)]
        d = [[r.integers(4, 300, size=r.integers(1, 30)) for _ in range(N)] for _ in range(B)]
        lab = r.integers(0, 2, size=(B, N))
        return ranker_batchify(flat_examples(q, d, lab, force_pad=(5, 29)), pin=True)
    b0, b1 = make(1), make(2)
    gp = GraphedPredictor(w, {k: v.cuda() for k, v in b0.items() if torch.is_tensor(v) and not k.startswith("_")})
    for b in (b1, b0, b1):
        before = gp.fast_path_calls
        got = gp.predict(b)
        assert gp.fast_path_calls == before + 1  # the packed single-memmove path was taken
        ref = w.predict({k: v for k, v in b.items() if torch.is_tensor(v) and not k.startswith("_")})
        assert torch.equal(got.cpu(), ref.cpu())


def test_validate_official_gpu_vs_oracle():
    """The evaluation driver on the HIP path gives the same MAP/MRR/P@k as the same loop over the CPU oracle."""
    from context_attentive_ir_amd.eval import validate_official
    from context_attentive_ir_amd.wrappers import Ranker
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    w = Ranker(default_args("MATCH_TENSOR", src_vocab_size=300))
    fill_module_(w.network, 13)
    sd = cpu_state_dict(w.network)
    w.cuda()
    rng = np.random.default_rng(8)
    batches = []
    for _ in range(5):
        q, ql, d, dl = _synth(rng, 6, 10, 4, 24, 300)
        lab = torch.zeros(6, 10, dtype=torch.int64)
        lab[torch.arange(6), torch.from_numpy(rng.integers(0, 10, size=6))] = 1
        batches.append({"que_rep": q, "que_len": ql, "doc_rep": d, "doc_len": dl, "label": lab})

    class OraclePredictor(object):
        def predict(self, ex):
            return torch.softmax(O.match_tensor_scores(sd, ex["que_rep"], ex["que_len"], ex["doc_rep"], ex["doc_len"]), -1)
    got = validate_official(batches, w)
    ref = validate_official(batches, OraclePredictor())
    assert got["examples"] == ref["examples"] == 30
    for k in ("map", "mrr", "prec@1", "prec@3", "prec@5"):
        assert abs(got[k] - ref[k]) < 1e-12, (k, got[k], ref[k])


def test_batches_in_flight_hint_keeps_results():
    """nir_set_stream_batches_in_flight only changes scheduling (no internal fork, 4-sequence recurrence layout): MatchTensor and
    CARS scores must stay within the parity tolerance of the oracle under either setting and agree with each other."""
    from context_attentive_ir_amd import lib
    L = lib.load()
    m = build_model("MATCH_TENSOR", vocab=300, device=DEV)
    rng = np.random.default_rng(31)
    q, ql, d, dl = [t.to(DEV) for t in _synth(rng, 9, 10, 4, 64, 300)]
    ref = O.match_tensor_scores(cpu_state_dict(m), q.cpu(), ql.cpu(), d.cpu(), dl.cpu())
    outs = []
    try:
        for n in (1, 4):
            lib.set_batches_in_flight(n)
            outs.append(m(q, ql, d, dl).cpu())
            _close(outs[-1], ref)
        other = torch.cuda.Stream()                       # the hint belongs to the stream it was set on: another stream is untouched
        with torch.cuda.stream(other):
            outs.append(m(q, ql, d, dl).cpu())
    finally:
        lib.set_batches_in_flight(0)
    _close(outs[0], outs[1], 2e-6)


def test_input_pipeline_end_to_end():
    """examples -> length-bucketed batches -> prefetched pinned single-buffer batches -> HIP scoring -> MAP/MRR/P@k,
    equal to the same loop over the CPU oracle (ragged shapes: every batch has its own QL/DL)."""
    from context_attentive_ir_amd.eval import validate_official
    from context_attentive_ir_amd.inputters import PrefetchingBatchStream, ranker_batchify, flat_examples, length_sorted_batches
    from context_attentive_ir_amd.wrappers import Ranker
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    w = Ranker(default_args("ESM", src_vocab_size=300))
    fill_module_(w.network, 17)
    sd = cpu_state_dict(w.network)
    w.cuda()
    rng = np.random.default_rng(12)
    n, N = 37, 5
    q = [rng.integers(4, 300, size=rng.integers(1, 6)) for _ in range(n)]
    d = [[rng.integers(4, 300, size=rng.integers(2, 40)) for _ in range(N)] for _ in range(n)]
    lab = np.zeros((n, N), dtype=np.int64)
    lab[np.arange(n), rng.integers(0, N, size=n)] = 1
    ex = flat_examples(q, d, lab)
    batches = length_sorted_batches([(max(len(x) for x in dd), len(qq)) for qq, dd in zip(q, d)], 8, rng=np.random.RandomState(4))

    class OraclePredictor(object):
        def predict(self, b):
            return torch.softmax(O.esm_scores(sd, b["que_rep"], b["que_len"], b["doc_rep"], b["doc_len"]), -1)
    got = validate_official(PrefetchingBatchStream(ex, batches, ranker_batchify, depth=2), w)
    ref = validate_official(PrefetchingBatchStream(ex, batches, ranker_batchify, depth=2, pin=False), OraclePredictor())
    assert got["examples"] == ref["examples"] == n
    for k in ("map", "mrr", "prec@1", "prec@3", "prec@5"):
        assert abs(got[k] - ref[k]) < 1e-12, (k, got[k], ref[k])


# ------------------------------------------------------------------ M_MATCH_TENSOR
def test_m_match_tensor_golden_and_oracle():
    """Session-aware MatchTensor ranking side: encode + rank_document vs the reference fixture, and vs the oracle on a
    ragged random batch through the Multitask wrapper (softmax over candidates)."""
    from context_attentive_ir_amd.wrappers import Multitask
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    g = load_golden("m_match_tensor")
    m = build_model("M_MATCH_TENSOR", tgt_vocab_size=int(g["tgt_vocab_size"]), device=DEV)
    src, sl, d, dl = (T(g[k], DEV) for k in ("source_words", "source_lens", "document_words", "document_lens"))
    pq, bank, states = m.encode(src, sl)
    _close(pq, g["projected_queries"])
    _close(m.rank_document(src, pq, bank, d, dl), g["scores"])
    # suggestion side (mmtensor.py:94-125, 281-325): session bank, decoder-initialisation states, greedy decode
    _close(bank, g["session_bank"], 1e-5); _close(states[0], g["dec_h"], 1e-5); _close(states[1], g["dec_c"], 1e-5)
    B_, S_ = src.shape[0], src.shape[1]
    dec = m.decode(states=states, max_len=int(g["max_len"]), src_dict=None, tgt_dict=None, batch_size=B_, session_len=S_ - 1, use_cuda=True,
                   tgt2src=T(g["tgt2src"], DEV))
    assert torch.equal(dec["predictions"].cpu(), T(g["predictions"]))

    w = Multitask(default_args("M_MATCH_TENSOR", src_vocab_size=300, tgt_vocab_size=40))
    fill_module_(w.network, 77)
    sd = cpu_state_dict(w.network)
    w.cuda()
    rng = np.random.default_rng(41)
    B, S, N, QL, DL = 3, 4, 6, 5, 40
    slen = rng.integers(1, QL + 1, size=(B, S)); dlen = rng.integers(1, DL + 1, size=(B, S, N))
    srcw = rng.integers(4, 300, size=(B, S, QL)); srcw[np.arange(QL)[None, None] >= slen[..., None]] = 0
    docw = rng.integers(4, 300, size=(B, S, N, DL)); docw[np.arange(DL)[None, None, None] >= dlen[..., None]] = 0
    ex = {"source_words": torch.from_numpy(srcw), "source_lens": torch.from_numpy(slen),
          "document_words": torch.from_numpy(docw), "document_lens": torch.from_numpy(dlen),
          "document_labels": torch.zeros(B, S, N)}
    res = w.predict(ex)                                        # the reference's predict always decodes (models/multitask.py:281-292)
    ref = torch.softmax(O.m_match_tensor_scores(sd, ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"]), -1)
    _close(res["click_scores"], ref)
    # greedy decode vs the oracle, with generator weights scaled up so that the arg-max moves between tokens
    sd2 = dict(sd)
    sd2["generator.weight"] = sd["generator.weight"] * 40.0
    w.network.load_state_dict(sd2)
    w.cuda()
    pq_o = O.m_match_tensor_encode(sd2, ex["source_words"], ex["source_lens"])
    m2 = O._strip_encoder_nesting(sd2)
    _, h_o, c_o = O.session_decoder_states(m2, "session_query_encoder", pq_o.max(1)[0].view(B, S, -1))
    lut = torch.from_numpy(np.random.default_rng(3).permutation(300)[:40].astype(np.int64))
    want = O.plain_greedy_decode(sd2, sd2["embedder.word_embeddings.make_embedding.emb_luts.0.weight"], h_o, c_o, 7, lut)
    _, _, st = w.network.encode(ex["source_words"].to(DEV), ex["source_lens"].to(DEV))
    _close(st[0], h_o, 1e-5)
    got = w.network.decode(states=st, max_len=7, src_dict=None, tgt_dict=None, batch_size=B, session_len=S - 1, tgt2src=lut.to(DEV))
    assert torch.equal(got["predictions"].cpu().view(-1, 7), want) and len(set(want.view(-1).tolist())) > 2
    assert tuple(w.predict(ex)["predictions"].shape) == (B, S - 1, w.args.max_query_len)


def test_m_match_tensor_state_dict_keys():
    """Reference checkpoints load with strict=True: the key set is the reference's (probed from neuroir M_MATCH_TENSOR)."""
    m = build_model("M_MATCH_TENSOR", tgt_vocab_size=50)
    keys = set(m.state_dict().keys())
    for k in ("embedder.word_embeddings.make_embedding.emb_luts.0.weight", "query_encoder.encoder.rnns.0.weight_hh_l0_reverse",
              "document_encoder.encoder.rnns.0.bias_ih_l0", "session_query_encoder.encoder.rnns.0.weight_ih_l0",
              "decoder.decoder.rnn.weight_hh_l0", "generator.weight", "exact_match_channel.alpha", "conv3.weight", "output.bias"):
        assert k in keys, k
    assert len(keys) == 44


# ------------------------------------------------------------------ MNSRF and the streaming recurrence
def test_mnsrf_golden_and_oracle():
    """MNSRF ranking side vs the reference fixture, then vs the oracle on a ragged random batch through the wrapper."""
    from context_attentive_ir_amd.wrappers import Multitask
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    g = load_golden("mnsrf")
    m = build_model("MNSRF", tgt_vocab_size=int(g["tgt_vocab_size"]), device=DEV)
    src, sl, d, dl = (T(g[k], DEV) for k in ("source_words", "source_lens", "document_words", "document_lens"))
    mem, sess, states = m.encode(src, sl)
    _close(mem, g["memory_bank"]); _close(sess, g["session_bank"])
    _close(m.rank_document(src, mem, sess, d, dl), g["scores"])
    _close(states[0], g["dec_h"], 1e-5); _close(states[1], g["dec_c"], 1e-5)       # suggestion side (mnsrf.py:88-112, 251-296)
    dec = m.decode(states=states, max_len=int(g["max_len"]), src_dict=None, tgt_dict=None, batch_size=src.shape[0], session_len=src.shape[1] - 1,
                   use_cuda=True, tgt2src=T(g["tgt2src"], DEV))
    assert torch.equal(dec["predictions"].cpu(), T(g["predictions"]))

    w = Multitask(default_args("MNSRF", src_vocab_size=300, tgt_vocab_size=40))
    fill_module_(w.network, 23)
    sd = cpu_state_dict(w.network)
    w.cuda()
    rng = np.random.default_rng(43)
    B, S, N, QL, DL = 3, 4, 5, 5, 21
    slen = rng.integers(1, QL + 1, size=(B, S)); dlen = rng.integers(1, DL + 1, size=(B, S, N))
    srcw = rng.integers(4, 300, size=(B, S, QL)); srcw[np.arange(QL)[None, None] >= slen[..., None]] = 0
    docw = rng.integers(4, 300, size=(B, S, N, DL)); docw[np.arange(DL)[None, None, None] >= dlen[..., None]] = 0
    ex = {"source_words": torch.from_numpy(srcw), "source_lens": torch.from_numpy(slen),
          "document_words": torch.from_numpy(docw), "document_lens": torch.from_numpy(dlen),
          "document_labels": torch.zeros(B, S, N)}
    res = w.predict(ex)
    ref = torch.softmax(O.mnsrf_scores(sd, ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"]), -1)
    _close(res["click_scores"], ref)
    assert len(w.network.state_dict()) == 29                  # the reference's key set (probed)
    assert tuple(res["predictions"].shape) == (B, S - 1, w.args.max_query_len)
    mem_o, _ = O.mnsrf_encode(sd, ex["source_words"], ex["source_lens"])
    m2 = O._strip_encoder_nesting(sd)
    _, h_o, c_o = O.session_decoder_states(m2, "session_query_encoder", mem_o)
    want = O.plain_greedy_decode(sd, sd["embedder.word_embeddings.make_embedding.emb_luts.0.weight"], h_o, c_o, w.args.max_query_len, None)
    assert torch.equal(res["predictions"].cpu().view(-1, w.args.max_query_len), want)


def _session_batches(n, B, S, N, QL, DL, V, seed, full=False):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        slen = rng.integers(1, QL + 1, size=(B, S)); dlen = rng.integers(1, DL + 1, size=(B, S, N))
        if full:
            slen[:] = QL; dlen[:] = DL
        srcw = rng.integers(4, V, size=(B, S, QL)); srcw[np.arange(QL)[None, None] >= slen[..., None]] = 0
        docw = rng.integers(4, V, size=(B, S, N, DL)); docw[np.arange(DL)[None, None, None] >= dlen[..., None]] = 0
        out.append({"source_words": torch.from_numpy(srcw), "source_lens": torch.from_numpy(slen),
                    "document_words": torch.from_numpy(docw), "document_lens": torch.from_numpy(dlen),
                    "document_labels": torch.zeros(B, S, N)})
    return out


@pytest.mark.parametrize("kind,shape", [("MNSRF", (3, 4, 5, 5, 21)), ("M_MATCH_TENSOR", (3, 4, 6, 5, 40)),
                                        ("MNSRF", (16, 7, 10, 4, 64)), ("M_MATCH_TENSOR", (16, 7, 10, 4, 64))])
def test_session_rankers_four_lanes_in_flight_equal_serial(kind, shape):
    """the captured Multitask.predict(suggest=False) graphs of 8 different batches, replayed with 4 lanes in flight, give
    BIT-identical probabilities to the same graphs replayed alone -- on the first replay after capture and in steady state -- and match
    the oracle within 1e-4 (small shapes; the X3 bench shape checks bit equality only).  The 0.2068 of profiles/r04_bench_detail.json
    was bench.py comparing never-replayed graphs' output buffers, not the library; this test pins the library side."""
    from context_attentive_ir_amd import lib
    from context_attentive_ir_amd.wrappers import Multitask
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    B, S, N, QL, DL = shape
    V = 300 if B < 16 else 20000
    w = Multitask(default_args(kind, src_vocab_size=V, tgt_vocab_size=40))
    fill_module_(w.network, 23)
    sd = cpu_state_dict(w.network)
    w.cuda()
    w.id_check_interval = 0
    exs = _session_batches(8, B, S, N, QL, DL, V, seed=len(kind) + B, full=B >= 16)
    dex = [{k: v.to(DEV) for k, v in ex.items()} for ex in exs]
    lanes = [torch.cuda.Stream() for _ in range(4)]
    lib.set_batches_in_flight(4, lanes)
    try:
        fn = lambda ex: w.predict(ex, suggest=False)["click_scores"]      # noqa: E731
        for i, ex in enumerate(dex):                                      # warm: packs, per-stream workspaces
            with torch.cuda.stream(lanes[i % 4]):
                fn(ex)
        torch.cuda.synchronize()
        graphs = []
        for i, ex in enumerate(dex):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=lanes[i % 4]):
                out = fn(ex)
            graphs.append((g, out))
        torch.cuda.synchronize()
        first, steady = None, None
        for rnd in range(6):                                              # all lanes in flight; round 0 = the first replay of every graph
            for i, (g, _) in enumerate(graphs):
                with torch.cuda.stream(lanes[i % 4]):
                    g.replay()
            if rnd == 0:
                torch.cuda.synchronize()
                first = [out.clone() for _, out in graphs]
        torch.cuda.synchronize()
        steady = [out.clone() for _, out in graphs]
        for i, (g, out) in enumerate(graphs):                             # each graph alone
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, first[i]), "%s graph %d: first concurrent replay differs from the serial replay by %g" % (
                kind, i, float((out - first[i]).abs().max()))
            assert torch.equal(out, steady[i]), "%s graph %d: concurrent replay differs from the serial replay by %g" % (
                kind, i, float((out - steady[i]).abs().max()))
            assert float(out.sum(-1).sub(1).abs().max()) < 1e-5
        if B < 16:
            score = O.mnsrf_scores if kind == "MNSRF" else O.m_match_tensor_scores
            for ex, got in zip(exs, steady):
                ref = torch.softmax(score(sd, ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"]), -1)
                _close(got, ref)
    finally:
        lib.set_batches_in_flight(0, lanes)


@pytest.mark.parametrize("H,I,M,T_,bi", [(256, 300, 9, 7, True), (200, 40, 5, 6, True), (1024, 64, 4, 5, False), (130, 300, 33, 4, True)])
def test_rnn_encoder_streaming_recurrence(H, I, M, T_, bi):
    """Hidden sizes beyond the register-resident kernels (H > 128): one GEMM + one cell kernel per step."""
    from context_attentive_ir_amd.encoders import RNNEncoder
    from context_attentive_ir_amd.detinit import fill_module_
    nd = 2 if bi else 1
    enc = fill_module_(RNNEncoder("LSTM", I, bi, 1, nd * H), seed=5).eval()
    g = torch.Generator().manual_seed(H + M)
    x = torch.randn(M, T_, I, generator=g); lens = torch.randint(1, T_ + 1, (M,), generator=g); lens[0] = T_
    sd = {"e." + k: v for k, v in enc.state_dict().items()}
    (hn_ref, cn_ref), ref = O.rnn_encode(sd, "e", x, lens, bidirectional=bi)
    enc = enc.to(DEV)
    (hn, cn), out = enc(x.to(DEV), lens.to(DEV))
    _close(out, ref, 3e-5)
    order = torch.sort(lens, 0, True)[1]
    _close(hn[:, order], hn_ref, 3e-5); _close(cn[:, order], cn_ref, 3e-5)


@pytest.mark.parametrize("kind", ["ESM", "MATCH_TENSOR", "DRMM", "DUET"])
def test_out_of_vocabulary_ids_raise_index_error(kind):
    """nn.Embedding raises IndexError for id >= V or < 0 (reference); the mirrors validate on the device (nir_sanitize_ids),
    keep running on PAD instead of reading out of bounds, and raise from check_ids()."""
    V = 300
    kw = dict(max_query_len=5, max_doc_len=20) if kind == "DUET" else {}
    m = build_model(kind, vocab=V, device=DEV, **kw)
    rng = np.random.default_rng(5)
    q, ql, d, dl = (t.to(DEV) for t in _synth(rng, 3, 4, 5, 20, V, full=True))
    good = m(q, ql, d, dl).clone()
    m.check_ids()
    for bad_id in (V, V + 12345, -1):
        bad = d.clone()
        bad[1, 2, 3] = bad_id
        out = m(q, ql, bad, dl)
        with pytest.raises(IndexError):
            m.check_ids()
        ref = d.clone(); ref[1, 2, 3] = 0
        _close(out, m(q, ql, ref, dl), 1e-6)            # the invalid id was scored as PAD, nothing was read out of bounds
    m.check_ids()                                           # flag cleared
    _close(m(q, ql, d, dl), good, 0)


# ------------------------------------------------------------------ full C4 batch (BASELINE configs[3]: 64 x 50 x doc_len 290)
def _c4_batch(V, QL=4, seed=1013):
    from context_attentive_ir_amd import synth
    return synth.ranker_batch(64, 50, QL, 290, V, seed, full_length=False)


def test_c4_full_batch_drmm_duet_esm():
    """The full C4 shape on one GPU: oracle parity on a slice of queries (the oracle materialises 4.45 GB tensors at the full
    batch), and size-independent properties on all 3200 pairs: scores of a query do not depend on the rest of the batch (batch
    slice == full batch), candidate permutation permutes scores, DUET stays inside (-2, 2), ESM inside [-1, 1]."""
    V = 20000
    ex = _c4_batch(V)
    dev = {k: v.to(DEV) for k, v in ex.items()}
    perm = torch.randperm(50, generator=torch.Generator().manual_seed(1))
    for kind, tol in (("ESM", 1e-4), ("DRMM", 5e-4), ("DUET", 1e-4)):
        kw = dict(max_query_len=4, max_doc_len=290) if kind == "DUET" else {}
        m = build_model(kind, vocab=V, device=DEV, **kw)
        full = m(dev["que_rep"], dev["que_len"], dev["doc_rep"], dev["doc_len"])
        assert full.shape == (64, 50) and torch.isfinite(full).all()
        sl = slice(5, 8)
        part = m(dev["que_rep"][sl], dev["que_len"][sl], dev["doc_rep"][sl], dev["doc_len"][sl])
        _close(part, full[sl], 1e-5 if kind != "DRMM" else 2e-4)
        permuted = m(dev["que_rep"], dev["que_len"], dev["doc_rep"][:, perm], dev["doc_len"][:, perm])
        _close(permuted, full[:, perm], 1e-5 if kind != "DRMM" else 2e-4)
        sd = cpu_state_dict(m)
        if kind == "DRMM":      # edge-safe comparison (Appendix E1): pairs whose histograms agree with the oracle's
            gate, cos, hist_ref = O.drmm_parts(sd, ex["que_rep"][sl], ex["doc_rep"][sl])
            _, hist = m(dev["que_rep"][sl], dev["que_len"][sl], dev["doc_rep"][sl], dev["doc_len"][sl], return_hist=True)
            hc = hist.cpu()
            assert (hc[..., :3] == hist_ref[..., :3]).all()        # only the two top bins are ambiguous (exact token overlaps, E1)
            same = (hc == hist_ref).all(-1).all(-1)
            ref = O.drmm_scores_from_hist(sd, gate, hist_ref, 3, 50).reshape(-1)
            assert same.any()                                      # Zipf ids at doc_len 290: most pairs share a token with the query
            _close(part.reshape(-1)[same], ref[same], tol)         # |scores| ~ 20..100: 5e-4 absolute = relative 1e-5
        else:
            ref = O.MODEL_FNS[kind](sd, ex["que_rep"][sl], ex["que_len"][sl], ex["doc_rep"][sl], ex["doc_len"][sl])
            _close(part, ref, tol)
        if kind == "DUET":
            assert float(full.abs().max()) < 2.0
        if kind == "ESM":
            assert float(full.abs().max()) <= 1.0 + 1e-6


@pytest.mark.parametrize("M,N,K", [(300, 300, 304), (1000, 300, 300), (5000, 130, 64), (13000, 256, 256)])
def test_linear_presplit_planes(M, N, K):
    """nir_split_f16x2 + nir_linear_planes_f32 (two-term fp16 planes, 3 MFMAs per product block) against fp64."""
    from context_attentive_ir_amd import lib
    g = torch.Generator().manual_seed(M + K)
    a = (torch.rand(M, K, generator=g) * 2 - 1).to(DEV); w = (torch.randn(N, K, generator=g) * 0.1).to(DEV); b = torch.randn(N, generator=g).to(DEV)
    KP = (K + 7) // 8 * 8
    a1, a2 = lib.split_f16x2(a, KP); w1, w2 = lib.split_f16x2(w, KP)
    c = torch.empty(M, N, device=DEV)
    lib.check(lib.load().nir_linear_planes_f32(lib.ptr(a1), lib.ptr(a2), KP, None, 0, 0, 0, 0, lib.ptr(w1), lib.ptr(w2), KP, lib.ptr(b), lib.ptr(c), N,
                                               M, N, KP, 1, lib.stream()), "planes")
    ref = torch.tanh(a.double() @ w.double().T + b.double()).float()
    _close(c, ref, 5e-6)


def test_duet_presplit_planes_path_matches_default():
    """DUET with pre-split table / conv-weight planes (conv_d1 gathers plane-table rows by id over 3 taps, the pooling kernel
    emits planes for conv_d2) against the default in-kernel split."""
    V = 600
    m = build_model("DUET", vocab=V, device=DEV, max_query_len=5, max_doc_len=40)
    rng = np.random.default_rng(2)
    q, ql, d, dl = (t.to(DEV) for t in _synth(rng, 3, 7, 5, 40, V, full=True))
    ref = m(q, ql, d, dl).clone()
    m.presplit_operands = True
    m._pack.invalidate()
    got = m(q, ql, d, dl)
    _close(got, ref, 5e-6)


@pytest.mark.parametrize("planes", [True, False])
@pytest.mark.parametrize("B,N,QL,DL,pool", [(2, 3, 4, 290, 5), (3, 5, 5, 64, 5), (1, 2, 3, 7, 5), (2, 2, 4, 131, 3), (1, 3, 4, 66, 1)])
def test_duet_fused_document_branch_matches_layer_chain(B, N, QL, DL, pool, planes):
    """The fused per-document-tile kernel (csrc/duet_fused.hip: conv_d1 -> pool -> conv_d2 -> Hadamard . fc2 on chip) against the
    GEMM-per-layer chain (tunable duet_unfused) and the oracle; tile counts 5 / 1 / 1 / 3 / 2 exercise the tile split and halos."""
    from context_attentive_ir_amd import lib
    V = 500
    m = build_model("DUET", vocab=V, device=DEV, max_query_len=QL, max_doc_len=DL, pool_size=pool)
    m.table_planes = planes          # True: token tile as fp16 term planes by LDS-direct loads; False: fp32 rows split in the kernel
    rng = np.random.default_rng(DL + pool)
    q, ql, d, dl = _synth(rng, B, N, QL, DL, V)
    qd, qld, dd, dld = (t.to(DEV) for t in (q, ql, d, dl))
    assert m._weights().struct.fw1 and m._weights().struct.K1P == 928 and bool(m._weights().struct.ftable) == planes
    s, loc, dist = m(qd, qld, dd, dld, return_parts=True)
    with lib.tunable("duet_unfused", 1, 0):
        s0, loc0, dist0 = m(qd, qld, dd, dld, return_parts=True)
    _close(dist, dist0, 5e-6)
    _close(s, s0, 5e-6)
    if planes:                       # 96-row tiles (documents of >= 98 - pool positions) against 64-row tiles
        with lib.tunable("duet_rows64", 1, 0):
            _close(m(qd, qld, dd, dld), s, 2e-6)
    if pool == 5:
        _close(dist, O.duet_distributed(cpu_state_dict(m), q, d))


@pytest.mark.parametrize("planes", [True, False])
@pytest.mark.parametrize("E,NF,DL,pool", [(52, 128, 150, 4), (100, 320, 97, 5), (300, 60, 200, 2), (64, 300, 290, 5),
                                         (448, 64, 150, 5), (640, 32, 120, 3)])   # wide rows: 64-row plane tiles / no room for the token tile -> fp32-table form
def test_duet_fused_other_widths(E, NF, DL, pool, planes):
    """Fused document branch away from the reference's 300/300/5: embedding width (k tail of conv_d1: 3E not a multiple of 32),
    filter count (masked columns, 320 = no padding), window, flattened and per-document tilings -- against the layer chain."""
    from context_attentive_ir_amd import lib
    V, B, N, QL = 400, 2, 3, 4
    m = build_model("DUET", vocab=V, device=DEV, max_query_len=QL, max_doc_len=DL, pool_size=pool, emsize=E, nfilters=NF)
    m.table_planes = planes
    rng = np.random.default_rng(E + NF)
    q, ql, d, dl = (t.to(DEV) for t in _synth(rng, B, N, QL, DL, V))
    assert m._weights().struct.fw1 and m._weights().struct.K1P == (3 * E + 31) // 32 * 32
    dist = m(q, ql, d, dl, return_parts=True)[2]
    with lib.tunable("duet_unfused", 1, 0):
        dist0 = m(q, ql, d, dl, return_parts=True)[2]
    _close(dist, dist0, 5e-6)


def test_embeddings_and_embedder_forward_match_nn_embedding():
    """modules.Embeddings.forward / multitask.layers.Embedder.forward (reference embeddings.py:243-252, layers.py:23-27): not on the hot path, but
    callable -- the HIP gather operator against torch's nn.Embedding, forward and the table gradient (PAD row excluded)."""
    from context_attentive_ir_amd.modules import Embeddings
    from context_attentive_ir_amd.multitask.layers import Embedder
    g = torch.Generator().manual_seed(2)
    V, E = 50, 12
    emb = Embeddings(E, V, 0).to(DEV)
    ref = torch.nn.Embedding(V, E, padding_idx=0)
    with torch.no_grad():
        w = torch.randn(V, E, generator=g); w[0] = 0
        emb.word_lut.weight.copy_(w.to(DEV)); ref.weight.copy_(w)
    ids = torch.randint(0, V, (3, 7), generator=g)
    out = emb(ids.unsqueeze(2).to(DEV))
    assert tuple(out.shape) == (3, 7, E) and torch.equal(out.cpu(), ref(ids))
    dout = torch.randn(3, 7, E, generator=g)
    out.backward(dout.to(DEV)); ref(ids).backward(dout)
    _close(emb.word_lut.weight.grad, ref.weight.grad, 1e-6)
    e2 = Embedder(E, V, 0.5).to(DEV).eval()
    with torch.no_grad():
        e2.word_embeddings.word_lut.weight.copy_(w.to(DEV))
    assert torch.equal(e2(ids.to(DEV)).cpu(), ref(ids).detach())          # eval: dropout off
    e2.train()
    y = e2(ids.to(DEV)).detach().cpu()
    kept = y != 0
    _close(y[kept], (ref(ids).detach() * 2.0)[kept], 1e-6)                # train: kept entries scaled by 1 / (1 - p)
    assert 0.2 < float(kept.float().mean()) < 0.8


@pytest.mark.parametrize("fold", [True, False])
def test_mnsrf_resident_recurrence_with_and_without_folded_tables(fold):
    """MNSRF at a shape where the cluster recurrence really runs for documents and queries (B*S*N = 240 documents of 21 tokens), against the ORACLE:
    folded gate tables (default) and fold_embeddings=False -- the same recurrence over per-batch gate rows written in the folded order by one
    gather-GEMM (ids == NULL) -- and that the kernels expected ran."""
    import ctypes as C
    from context_attentive_ir_amd import lib
    from context_attentive_ir_amd.wrappers import Multitask
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    w = Multitask(default_args("MNSRF", src_vocab_size=300, tgt_vocab_size=40, fold_embeddings=fold))
    fill_module_(w.network, 29)
    sd = cpu_state_dict(w.network)
    w.cuda()
    ex = _session_batches(1, 6, 5, 8, 5, 21, 300, seed=3)[0]
    L = lib.load()
    res = w.predict(ex, suggest=False)["click_scores"]
    L.nir_profile_enable(1)
    res2 = w.predict(ex, suggest=False)["click_scores"]
    torch.cuda.synchronize()
    L.nir_profile_enable(0)
    buf = C.create_string_buffer(1 << 16)
    L.nir_profile_report(buf, len(buf))
    names = {ln.rsplit(",", 2)[0].split("[")[0] for ln in buf.value.decode().strip().splitlines()}
    assert "lstm_cluster_kernel" in names and "lstm_step_cell_kernel" not in names, names
    assert (w.network._weights().struct.d_fold is not None) == fold
    assert torch.equal(res, res2)
    ref = torch.softmax(O.mnsrf_scores(sd, ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"]), -1)
    _close(res, ref)
    w.network.check_ids()
