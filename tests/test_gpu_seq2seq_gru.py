"""GPU (-m gpu): Seq2seqGRU (csrc/gru_step.hip, csrc/seq2seq.hip, recommender/seq2seq_gru.py, wrappers/recommender.py) against the
reference's recorded decode, loss and update losses with rnn_type = 'GRU' (tests/golden/seq2seq_gru.npz) and against the fp64 restatement of
tests/gru_dec_ref.py: every fixture case, exact tokens, the bound on the attentions, the fast and the plain step against each other, eager
predict against graph replay, bitwise repeatability, train mode (loss, every gradient, recorded update losses), and autograd.gru_seq with an
initial state against torch.nn.GRU in float64."""
import numpy as np
import pytest
import torch

import gru_dec_ref as R
from conftest import T

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = R.golden("s2s")
SRC, LENS = T(G["source_words"]), T(G["source_lens"])
QL, MAXLEN, VT = SRC.shape[1], int(G["max_len"]), int(G["tgt_vocab"])
SPECIAL = ["<blank>", "<unk>", "<s>", "</s>"]
TGT_DICT = [SPECIAL[i] if i < 4 else "w%d" % i for i in range(VT)]
SRC_DICT = {TGT_DICT[i]: int(s) for i, s in enumerate(G["tgt2src"])}        # src_dict[tgt_dict[i]] = tgt2src[i]


def _wrap(tag, **kw):
    from context_attentive_ir_amd.recommender import Seq2seqGRU
    from context_attentive_ir_amd.wrappers import Recommender
    net = R.case("s2s", tag)[0]
    r = Recommender(R.case_args("s2s", tag, **kw), SRC_DICT, TGT_DICT, net.state_dict())
    assert type(r.network) is Seq2seqGRU
    r.cuda()
    r.network.eval()
    return r


@pytest.fixture(scope="module")
def cases():
    """every fixture case once: (wrapper on the GPU, cfg, golden arrays, fp64 decode, fp32 decode)"""
    out = {}
    for tag in R.S2S_CASES:
        net, c, g = R.case("s2s", tag)
        sd, lut = net.state_dict(), T(g["tgt2src"])
        out[tag] = (_wrap(tag), c, g, R.decode(sd, c, SRC, LENS, MAXLEN, lut), R.decode(sd, c, SRC, LENS, MAXLEN, lut, torch.float32))
    return out


def _decode(net):
    return net.decode(SRC.to(DEV), LENS.to(DEV), MAXLEN, SRC_DICT, TGT_DICT)


def _n_split(net):
    """split products on the path of the last attention row: one per step on the fast step"""
    return MAXLEN if net._decoder_weights().struct.rnn_whh_frag else 0


@pytest.mark.parametrize("tag", R.S2S_CASES)
def test_decode_matches_the_reference_and_the_fp64_bound(cases, tag):
    r, c, g, ref, chain = cases[tag]
    net = r.network
    got = _decode(net)
    assert got["predictions"].shape == (SRC.shape[0], MAXLEN) and got["attentions"].shape == (SRC.shape[0], MAXLEN, QL)
    assert torch.equal(got["predictions"].cpu(), T(g["predictions"]))
    w = net._decoder_weights().struct
    assert w.gen_frag and w.rnn_whh_frag and w.rnn_gate_fold          # detinit weights are far inside the split range: the fast step ran
    ok, fig = R.accept_decode(got, ref, chain, _n_split(net))
    print("seq2seq_gru bound %s: %s" % (tag, fig))
    assert ok, fig
    assert float((got["attentions"].cpu() - R.pad_attn(g["attentions"], QL)).abs().max()) <= 1e-4
    masked = (torch.arange(QL).view(1, 1, QL) >= LENS.view(-1, 1, 1)).expand(-1, MAXLEN, -1)
    assert bool((got["attentions"].cpu()[masked] == 0).all())
    again = _decode(net)
    assert torch.equal(again["predictions"], got["predictions"]) and torch.equal(again["attentions"], got["attentions"])


@pytest.mark.parametrize("tag", R.S2S_CASES)
def test_fast_and_plain_step_agree_on_the_tokens(cases, tag):
    r, c, g, ref, chain = cases[tag]
    net = r.network
    try:
        for fold, fuse in ((False, True), (False, False)):
            net.fold_decoder_step, net.fuse_generator_argmax = fold, fuse
            w = net._decoder_weights().struct
            assert not w.rnn_whh_frag and not w.rnn_gate_fold and bool(w.gen_frag) == fuse
            got = _decode(net)
            ok, fig = R.accept_decode(got, ref, chain, 0)
            print("seq2seq_gru bound %s plain step fuse=%s: %s" % (tag, fuse, fig))
            assert ok, fig
            assert torch.equal(got["predictions"].cpu(), T(g["predictions"]))
    finally:
        net.fold_decoder_step = net.fuse_generator_argmax = True


@pytest.mark.parametrize("tag", R.S2S_CASES)
def test_predict_eager_then_graph_replay(cases, tag):
    r, c, g, ref, chain = cases[tag]
    r.predict_graph_min_calls = 2
    r.clear_predict_graphs()
    ex = dict(source_words=SRC.unsqueeze(1), source_lens=LENS.unsqueeze(1))
    a = r.predict(ex)                                                   # eager
    b = r.predict(ex)                                                   # captured and replayed
    d = r.predict(ex)                                                   # replayed
    assert r._graphs is not None and r._graphs.captures == 1 and r._graphs.replays >= 2
    for o in (a, b, d):
        assert torch.equal(o["prediction_ids"].cpu(), T(g["predictions"]))
        assert torch.equal(o["attentions"], a["attentions"])


# ---- train mode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", R.S2S_CASES)
def test_loss_and_gradients_against_fp64(tag):
    net, c, g = R.case("s2s", tag)
    net = net.to(DEV)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net.dec_dropout_p = 0.0
    net.train()
    tw, ts, tl = T(G["target_words"]), T(G["target_seq"]), T(G["target_lens"])
    loss = net(SRC.to(DEV), LENS.to(DEV), tw.to(DEV), tl.to(DEV), ts.to(DEV), None, None)
    loss.backward()
    print("seq2seq_gru loss %s: %.7f (reference %.7f)" % (tag, float(loss), float(g["loss"])))
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    params = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    p = dict(params)
    p[R.S.EMB] = torch.cat([params[R.S.EMB][:1].detach(), params[R.S.EMB][1:]], 0)          # nn.Embedding(padding_idx=PAD): no gradient for the PAD row
    ref = R.loss(p, c, SRC, LENS, tw, ts)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    for name, prm in net.named_parameters():
        gr = params[name].grad
        assert prm.grad is not None, name
        err = (prm.grad.cpu().double() - gr).abs().max() / max(float(gr.abs().max()), 1e-5)
        print("seq2seq_gru grad %s %s: %.3g" % (tag, name, float(err)))
        assert float(err) < 1e-4, (name, float(err))


@pytest.mark.parametrize("fix", [True, False])
def test_recorded_update_losses(fix):
    from context_attentive_ir_amd.wrappers import Recommender
    net = R.case("s2s", "general")[0]
    r = Recommender(R.case_args("s2s", "general", dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0,
                                momentum=0, grad_clipping=10.0, fix_embeddings=fix), list(range(int(G["vocab"]))), list(range(VT)), net.state_dict())
    r.cuda()
    r.init_optimizer()
    batches = [{k: T(G["train_b%d_%s" % (bi, k)]) for k in ("source_words", "source_lens", "target_words", "target_seq", "target_lens")}
               for bi in range(2)]
    losses = [float(r.update(batches[step % 2])) for step in range(3)]
    print("seq2seq_gru update losses (fix_embeddings=%s): %s" % (fix, losses))
    np.testing.assert_allclose(losses, G["train_losses_" + ("fix" if fix else "free")], rtol=1e-4, atol=0)
    # decode at the new weights: a stale pack would miss the bound against the network's own state dict
    r.network.eval()
    c = R.case_cfg("s2s", "general")
    sd = {k: v.cpu() for k, v in r.network.state_dict().items()}
    ref, chain = R.decode(sd, c, SRC, LENS, MAXLEN), R.decode(sd, c, SRC, LENS, MAXLEN, dtype=torch.float32)
    assert float(ref["gaps"].min()) >= 1e-4, "the updated weights' own logit gaps are too small to compare tokens: %s" % ref["gaps"].min()
    got = r.network.decode(SRC.to(DEV), LENS.to(DEV), MAXLEN, None, None)
    ok, fig = R.accept_decode(got, ref, chain, _n_split(r.network))
    assert ok, fig


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("Tn", [1, 6])
@pytest.mark.parametrize("H", [32, 160])
def test_gru_seq_with_an_initial_state_against_torch(M, Tn, H):
    from context_attentive_ir_amd import autograd as A
    I = 12
    g = torch.Generator().manual_seed(100 * M + 10 * Tn + H)
    ref = torch.nn.GRU(I, H, 1, batch_first=True).double()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (0.5 if p.dim() == 1 else H ** -0.5))
    x = torch.randn(M, Tn, I, generator=g, dtype=torch.float64, requires_grad=True)
    h0 = torch.tanh(torch.randn(M, H, generator=g, dtype=torch.float64)).requires_grad_(True)
    wout = torch.randn(M, Tn, H, generator=g, dtype=torch.float64)
    out, _ = ref(x, h0.unsqueeze(0))
    (out * wout).sum().backward()
    gru = torch.nn.GRU(I, H, 1, batch_first=True).to(DEV)
    gru.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    xd = x.detach().float().to(DEV).requires_grad_(True)
    hd = h0.detach().float().to(DEV).requires_grad_(True)
    got = A.gru_seq(xd, gru, hd)
    (got * wout.float().to(DEV)).sum().backward()
    rel = lambda a, b: float((a.detach().cpu().double() - b).abs().max() / max(float(b.abs().max()), 1e-5))          # noqa: E731
    figs = dict(fwd=rel(got, out.detach()), dh0=rel(hd.grad, h0.grad), dwhh=rel(gru.weight_hh_l0.grad, ref.weight_hh_l0.grad),
                dx=rel(xd.grad, x.grad), dbhh=rel(gru.bias_hh_l0.grad, ref.bias_hh_l0.grad), dwih=rel(gru.weight_ih_l0.grad, ref.weight_ih_l0.grad))
    print("gru_seq h0 M=%d T=%d H=%d: %s" % (M, Tn, H, figs))
    assert figs["fwd"] <= 1e-5, figs
    assert max(figs["dh0"], figs["dwhh"], figs["dx"], figs["dbhh"], figs["dwih"]) <= 1e-4, figs
    # without h0 the call is the one it was: the zero state, the same bits as a zero h0 gives
    a = A.gru_seq(xd.detach(), gru)
    b = A.gru_seq(xd.detach(), gru, torch.zeros(M, H, device=DEV))
    assert float((a - b).abs().max()) <= 1e-6
