"""GPU (-m gpu): the train-mode GRU and the stacked encoders -- nir_gru_train_fwd / _bwd (both BPTT forms), the streaming cell kernels, RNNEncoder.forward_train
and MatchTensor training with GRU / stacked encoders -- against the float64 restatement (tests/rnn_train_ref.py) and the reference's recorded training
steps (tests/golden/match_tensor_rnn_train.npz).  Bars: the project's own (tests/test_gpu_train.py): outputs 2e-5, gradients 1e-4 of the largest
entry (floor 1e-5), losses 1e-5, trajectories rtol 1e-4, graphed against eager rtol 2e-5."""
import numpy as np
import pytest
import torch

import rnn_train_ref as R
from conftest import T, load_golden
from helpers import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = {"gru1": ("GRU", 1), "gru2": ("GRU", 2), "lstm2": ("LSTM", 2)}
TRAIN_KW = dict(dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0, momentum=0, grad_clipping=10.0,
                fix_embeddings=True)


def _rel(a, b, tol=1e-4, floor=1e-5, what=""):
    err = R.rel_err(a, b, floor)
    print("%s relative error %.3g (bar %.3g)" % (what, err, tol))
    assert err <= tol, "%s relative error %.3g > %.3g" % (what, err, tol)


def _module(cell, layer, bi):
    H, I = layer["weight_hh_l0"].shape[1], layer["weight_ih_l0"].shape[1]
    m = getattr(torch.nn, cell)(I, H, 1, bidirectional=bi, batch_first=True)
    m.load_state_dict({k: v.float() for k, v in layer.items()})
    return m.to(DEV)


def _check_layer(mod, xd, out, ref, what):
    _rel(out, ref[0], 2e-5, what=what + " bank")
    _rel(xd.grad, ref[1], what=what + " dx")
    for k, p in mod.named_parameters():
        _rel(p.grad, ref[2][0][k], what=what + " " + k)


def _run_birnn(shape, configs):
    from context_attentive_ir_amd import autograd as A
    H, I, M, T_, bi = shape
    layers, x, lens, dout = R.make_case(*shape)
    ref = R.gru_stack(layers, x, lens, dout, bi)
    gru = _module("GRU", layers[0], bi)
    xd = x.float().to(DEV).requires_grad_(True)
    for packed, form in configs:
        A.PACKED_WGRAD, A.GRU_FORM = packed, form
        try:
            gru.zero_grad(); xd.grad = None
            out = A.birnn(xd, lens.to(DEV), gru)
            out.backward(dout.float().to(DEV))
        finally:
            A.PACKED_WGRAD, A.GRU_FORM = False, 0
        _check_layer(gru, xd, out, ref, "%s packed=%d form=%d" % (shape, packed, form))


@pytest.mark.parametrize("shape", R.SHAPES)
def test_bigru_backward(shape):
    """register-resident recurrence + BPTT: the library's dispatch, the VALU form and (where it takes the shape) the matrix-core form, each forced
    once; the weight gradients over all rows and over the list of valid rows"""
    from context_attentive_ir_amd import lib
    configs = [(False, 0), (True, 1)]
    if lib.load().nir_gru_train_mfma_supported(shape[0]):
        configs.append((False, 2))
    _run_birnn(shape, configs)


@pytest.mark.parametrize("shape", R.SEQ_SHAPES)
def test_gru_streaming_form_backward(shape):
    """beyond 128 units per direction: one recurrent GEMM + one cell kernel per step (autograd._GRUSeq), the reverse direction gathered"""
    _run_birnn(shape, [(False, 0)])


def _abi_case(H, I, M, T_, bi, lens):
    """one layer through the C ABI -> (layer, x, lens, dout, reference, {form: (out, hn, dgx, dq)}); every output buffer starts as NaN"""
    from context_attentive_ir_amd import lib
    L = lib.load()
    layers, x, _, dout = R.make_case(H, I, M, T_, bi)
    lens = torch.as_tensor(lens, dtype=torch.int64)
    ref = R.gru_stack(layers, x, lens.clamp(0, T_), dout, bi)          # (the kernels clamp lengths to [0, T])
    p, nd = layers[0], (2 if bi else 1)
    sfx = ["", "_reverse"][:nd]
    dev = lambda t: t.float().contiguous().to(DEV)                                                 # noqa: E731
    wih, bih = dev(torch.cat([p["weight_ih_l0" + s] for s in sfx], 0)), dev(torch.cat([p["bias_ih_l0" + s] for s in sfx], 0))
    whh, bhh = dev(torch.stack([p["weight_hh_l0" + s] for s in sfx], 0)), dev(torch.stack([p["bias_hh_l0" + s] for s in sfx], 0))
    gin = (dev(x).reshape(M * T_, I) @ wih.t() + bih).contiguous()
    ld, dd = lens.to(DEV), dev(dout)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)                                       # noqa: E731
    res = {}
    for form in (1, 2) if L.nir_gru_train_mfma_supported(H) else (1,):
        out, act, hn = nan(M, T_, nd * H), nan(M, T_, nd, 4 * H), nan(nd, M, H)
        dgx, dq = nan(M, T_, nd * 3 * H), nan(M, T_, nd * H)
        lib.check(L.nir_gru_train_fwd(lib.ptr(gin), lib.ptr(ld), lib.ptr(whh), lib.ptr(bhh), lib.ptr(out), lib.ptr(act), lib.ptr(hn), M, T_, H, nd, lib.stream()),
                  "nir_gru_train_fwd")
        lib.check(L.nir_gru_train_bwd(lib.ptr(dd), None, lib.ptr(act), lib.ptr(out), lib.ptr(ld), lib.ptr(whh), lib.ptr(dgx), lib.ptr(dq), M, T_, H, nd, form,
                                      lib.stream()), "nir_gru_train_bwd")
        torch.cuda.synchronize()
        res[form] = tuple(t.cpu() for t in (out, hn, dgx, dq))
    return layers[0], x, lens, dout, ref, res


@pytest.mark.parametrize("H,I,M,T_,bi,lens", [(15, 8, 6, 5, True, [5, 0, 3, 1, 0, 2]), (64, 8, 18, 4, True, [4, 0, 2] * 6), (32, 8, 5, 1, True, [1, 0, 1, 1, 1]),
                                              (70, 12, 19, 6, True, [1] * 19), (20, 8, 3, 4, False, [9, -2, 4])])
def test_c_abi_edge_cases(H, I, M, T_, bi, lens):
    """zero-length rows (zero out / gradient rows, zero hn), T = 1, all lengths 1, lengths clamped to [0, T]; both BPTT forms; every position of
    out / dgx / dq is written (the buffers start as NaN)"""
    layer, x, lens, dout, ref, res = _abi_case(H, I, M, T_, bi, lens)
    nd = 2 if bi else 1
    cl = lens.clamp(0, T_)
    wih = torch.cat([layer["weight_ih_l0" + s] for s in ["", "_reverse"][:nd]], 0)
    for form, (out, hn, dgx, dq) in res.items():
        assert bool(torch.isfinite(out).all() and torch.isfinite(dgx).all() and torch.isfinite(dq).all() and torch.isfinite(hn).all()), form
        for m in range(M):
            n = int(cl[m])
            assert float(out[m, n:].abs().max() if n < T_ else 0) == 0 and float(dgx[m, n:].abs().max() if n < T_ else 0) == 0
            assert float(dq[m, n:].abs().max() if n < T_ else 0) == 0
            if n == 0:
                assert float(hn[:, m].abs().max()) == 0
            else:                                                      # the final state: the last valid step (forward), position 0 (reverse)
                assert torch.equal(hn[0, m], out[m, n - 1, :H]) and (nd == 1 or torch.equal(hn[1, m], out[m, 0, H:]))
        _rel(out, ref[0], 2e-5, what="form %d bank" % form)
        _rel(dgx.double().reshape(M * T_, -1) @ wih, ref[1].reshape(M * T_, -1), what="form %d dx" % form)
        for di, s in enumerate(["", "_reverse"][:nd]):
            _rel(dgx[:, :, di * 3 * H:(di + 1) * 3 * H].double().sum((0, 1)), ref[2][0]["bias_ih_l0" + s], what="form %d db_ih%s" % (form, s))
            dbhh = torch.cat((dgx[:, :, di * 3 * H:di * 3 * H + 2 * H].double().sum((0, 1)), dq[:, :, di * H:(di + 1) * H].double().sum((0, 1))))
            _rel(dbhh, ref[2][0]["bias_hh_l0" + s], what="form %d db_hh%s" % (form, s))
    if len(res) == 2:                                                  # deterministic kernels: a second run of one form gives the same bits
        again = _abi_case(H, I, M, T_, bi, lens.tolist())[5]
        for form in res:
            assert all(torch.equal(a, b) for a, b in zip(res[form], again[form])), form


def test_c_abi_empty_batch_enqueues_nothing():
    from context_attentive_ir_amd import lib
    L = lib.load()
    buf = torch.full((64,), 7.0, device=DEV)
    p = lib.ptr(buf)
    assert L.nir_gru_train_fwd(p, None, p, p, p, p, p, 0, 3, 8, 2, lib.stream()) == 0
    for form in (0, 1, 2):
        assert L.nir_gru_train_bwd(p, None, p, p, None, p, p, p, 0, 3, 32, 2, form, lib.stream()) == 0
    assert L.nir_gru_cell_seq_fwd(p, 24, p, p, None, 0, p, 32, p, 8, 0, 8, lib.stream()) == 0
    assert L.nir_gru_cell_seq_bwd(p, 8, None, None, p, 32, None, 0, p, 24, p, 24, p, 0, 8, lib.stream()) == 0
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


def _encoder(cell, layers, bi, dropout=0.0, use_last=True):
    from context_attentive_ir_amd.encoders.rnn_encoder import RNNEncoder
    H, I = layers[0]["weight_hh_l0"].shape[1], layers[0]["weight_ih_l0"].shape[1]
    enc = RNNEncoder(cell, I, bi, len(layers), H * (2 if bi else 1), dropout, use_last=use_last)
    enc.load_state_dict({"rnns.%d.%s" % (i, k): v.float() for i, p in enumerate(layers) for k, v in p.items()})
    return enc.to(DEV)


@pytest.mark.parametrize("cell,bi,nl,use_last", [("GRU", True, 2, True), ("LSTM", True, 2, True), ("GRU", False, 3, True), ("GRU", True, 2, False)])
def test_forward_train_stacked_layers(cell, bi, nl, use_last):
    H, I, M, T_ = 24, 8, 9, 9
    layers, x, lens, dout = R.make_case(H, I, M, T_, bi, nlayers=nl, gates=3 if cell == "GRU" else 4, use_last=use_last)
    ref = (R.gru_stack(layers, x, lens, dout, bi, use_last=use_last) if cell == "GRU" else R.torch_stack(layers, x, lens, dout, bi, cell="LSTM", use_last=use_last))
    enc = _encoder(cell, layers, bi, use_last=use_last).train()
    xd = x.float().to(DEV).requires_grad_(True)
    bank = enc.forward_train(xd, lens.to(DEV))
    bank.backward(dout.float().to(DEV))
    what = "%s bi=%d layers=%d" % (cell, bi, nl)
    _rel(bank, ref[0], 2e-5, what=what + " bank")
    _rel(xd.grad, ref[1], what=what + " dx")
    for li in range(nl):
        for k, v in ref[2][li].items():
            _rel(enc.rnns[li].get_parameter(k).grad, v, what="%s layer %d %s" % (what, li, k))
    with torch.no_grad():
        ev = enc.eval()(x.float().to(DEV), lens.to(DEV))[1]
    _rel(bank, ev, 2e-5, what=what + " train bank against the eval path")


def test_forward_train_inter_layer_dropout():
    from context_attentive_ir_amd import autograd as A
    H, I, M, T_, p_drop = 24, 8, 9, 9, 0.3
    layers, x, lens, dout = R.make_case(H, I, M, T_, True, nlayers=2)
    enc = _encoder("GRU", layers, True, dropout=p_drop).train()
    xd = x.float().to(DEV).requires_grad_(True)
    dd = dout.float().to(DEV)

    def loss(seed):
        A.DROPOUT.manual_seed(seed)
        with torch.no_grad():
            return float((enc.forward_train(xd, lens.to(DEV)) * dd).sum())
    l1, l2, l1b = loss(5), loss(6), loss(5)
    assert l1 == l1b and abs(l1 - l2) > 1e-3 * abs(l1), (l1, l2, l1b)
    A.DROPOUT.manual_seed(5)
    A.DROPOUT.record, A.DROPOUT.masks = True, []
    try:
        bank = enc.forward_train(xd, lens.to(DEV))
    finally:
        A.DROPOUT.record = False
    masks = [k.cpu().bool() for k in A.DROPOUT.masks]
    assert len(masks) == 1 and tuple(masks[0].shape) == (M, T_, 2 * H) and 0.6 < float(masks[0].float().mean()) < 0.8
    bank.backward(dd)
    ref = R.gru_stack(layers, x, lens, dout, True, masks=[None, masks[0]], p_drop=p_drop)
    _rel(bank, ref[0], 2e-5, what="dropout bank")
    _rel(xd.grad, ref[1], what="dropout dx")
    for li in range(2):
        for k, v in ref[2][li].items():
            _rel(enc.rnns[li].get_parameter(k).grad, v, what="dropout layer %d %s" % (li, k))


# ------------------------------------------------------------------ MatchTensor with GRU / stacked encoders: the reference's recorded training steps
def _batch(g, tag, i, dev="cpu"):
    return {k: T(g["%s.b%d_%s" % (tag, i, k)], dev) for k in ("que_rep", "que_len", "doc_rep", "doc_len", "label")}


def _ranker(g, tag):
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import Ranker
    rnn_type, nlayers = CASES[tag]
    r = Ranker(default_args("MATCH_TENSOR", src_vocab_size=int(g["meta_vocab"]), rnn_type=rnn_type, nlayers=nlayers, **TRAIN_KW))
    fill_module_(r.network, 1013)
    r.cuda()
    r.init_optimizer()
    return r


@pytest.mark.parametrize("tag", sorted(CASES))
def test_match_tensor_rnn_gradients_vs_reference(tag):
    from context_attentive_ir_amd import autograd as A
    g = load_golden("match_tensor_rnn_train")
    rnn_type, nlayers = CASES[tag]
    m = build_model("MATCH_TENSOR", vocab=int(g["meta_vocab"]), device=DEV, dropout_emb=0.0, dropout_rnn=0.0, rnn_type=rnn_type, nlayers=nlayers).train()
    m.word_embeddings.table.requires_grad_(False)
    b = _batch(g, tag, 0, DEV)
    s = m(b["que_rep"], b["que_len"], b["doc_rep"], b["doc_len"])
    _rel(s, g[tag + ".scores0"], 2e-5, what=tag + " scores0")
    loss = A.bce_with_logits(s, b["label"].float())
    _rel(loss, g[tag + ".loss0"], 1e-5, what=tag + " loss0")
    loss.backward()
    for name, p in m.named_parameters():
        if not p.requires_grad:
            continue
        if "%s.grad_%s" % (tag, name) in g:
            _rel(p.grad, g["%s.grad_%s" % (tag, name)], what=tag + " " + name)
        else:                                      # large tensors are stored as every 37th element + the norm
            _rel(p.grad.flatten()[::37], g["%s.gradsub37_%s" % (tag, name)], what=tag + " " + name + " [::37]")
            _rel(p.grad.norm(), g["%s.gradnorm_%s" % (tag, name)], what=tag + " " + name + " norm")


@pytest.mark.parametrize("tag", sorted(CASES))
def test_ranker_update_rnn_matches_reference_loss_trajectory(tag):
    g = load_golden("match_tensor_rnn_train")
    r = _ranker(g, tag)
    losses = [float(r.update(_batch(g, tag, step % 2))) for step in range(5)]
    print(tag, "losses", losses, "reference", g[tag + ".losses"].tolist())
    np.testing.assert_allclose(np.asarray(losses), g[tag + ".losses"], rtol=1e-4, atol=0)
    assert r.updates == 5


def test_graphed_update_reproduces_the_eager_gru_trajectory_and_predict_follows():
    """gru1: six captured updates leave the losses and parameters of six eager ones; predict() afterwards scores the trained weights (equal to a fresh
    model loaded with the same state dict), not those of the capture"""
    from context_attentive_ir_amd.wrappers import GraphedUpdate
    g = load_golden("match_tensor_rnn_train")
    batches = [_batch(g, "gru1", i, DEV) for i in range(2)]
    finals = []
    for graphed in (False, True):
        w = _ranker(g, "gru1")
        before = w.predict(batches[0]).cpu()
        step = GraphedUpdate(w) if graphed else w.update
        losses = [float(step(batches[i % 2])) for i in range(6)]
        finals.append((losses, {k: v.detach().clone() for k, v in w.network.state_dict().items()}, w.updates, before, w.predict(batches[0]).cpu()))
    (le, pe, ue, _, _), (lg, pg, ug, before, after) = finals
    assert ue == ug == 6
    print("eager", le, "graphed", lg)
    np.testing.assert_allclose(lg, le, rtol=2e-5)
    for k in pe:      # (Adam turns rounding differences of near-zero gradients into parameter differences of a few 1e-5 over six steps: test_gpu_train.py)
        assert float((pe[k] - pg[k]).abs().max()) <= 1e-4 * max(1.0, float(pe[k].abs().max())), k
    fresh = _ranker(g, "gru1")
    fresh.network.load_state_dict(pg)
    fresh.args.predict_graphs = False
    want = fresh.predict(batches[0]).cpu()
    assert float((after - before).abs().max()) > 1e-4                  # the six steps moved the scores
    assert float((after - want).abs().max()) < 1e-6, float((after - want).abs().max())
