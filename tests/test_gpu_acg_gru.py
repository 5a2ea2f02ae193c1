"""GPU (-m gpu): ACGGRU (csrc/gru_step.hip in front of csrc/acg.hip's copy generator, recommender/seq2seq_gru.py, wrappers.CopyRecommender)
against the reference's recorded decode, copy losses and update losses with rnn_type = 'GRU' (tests/golden/seq2seq_gru.npz) and against the
fp64 restatement of tests/gru_dec_ref.py: the three fixture cases on the fast and the plain step, exact tokens including copied and collapsed
winners, attentions, bitwise repeatability, eager predict against graph replay, train mode (copy loss, every gradient, recorded update
losses)."""
import numpy as np
import pytest
import torch

import acg_ref as AR
import gru_dec_ref as R
from conftest import T

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = R.golden("acg")
D = R.acg_batch()
SRC, LENS = D["src"], D["lens"]
QL, MAXLEN, VT = SRC.shape[1], int(G["max_len"]), int(G["tgt_vocab"])
E2T, E2S = AR.index_tensors(D)


def _wrap(tag, **kw):
    from context_attentive_ir_amd.recommender import ACGGRU
    from context_attentive_ir_amd.wrappers import CopyRecommender
    net = R.case("acg", tag)[0]
    r = CopyRecommender(R.case_args("acg", tag, **kw), D["src_dict"], D["tgt_dict"], net.state_dict())
    assert type(r.network) is ACGGRU
    r.cuda()
    r.network.eval()
    return r


@pytest.fixture(scope="module")
def cases():
    """every fixture case once: (wrapper on the GPU, cfg, golden arrays, fp64 decode, fp32 decode)"""
    out = {}
    for tag in R.ACG_CASES:
        net, c, g = R.case("acg", tag)
        sd = net.state_dict()
        out[tag] = (_wrap(tag), c, g, R.acg_decode(sd, c, SRC, LENS, MAXLEN, D["idx"], E2T, E2S),
                    R.acg_decode(sd, c, SRC, LENS, MAXLEN, D["idx"], E2T, E2S, dtype=torch.float32))
    return out


def _decode(net):
    return net.decode(SRC.to(DEV), LENS.to(DEV), MAXLEN, D["src_dict"], D["tgt_dict"], src_map_idx=D["idx"], ext2tgt=E2T, ext2src=E2S)


@pytest.mark.parametrize("fold", [True, False], ids=["fast", "plain"])
@pytest.mark.parametrize("tag", R.ACG_CASES)
def test_decode_matches_the_reference(cases, tag, fold):
    r, c, g, ref, chain = cases[tag]
    net = r.network
    net.fold_decoder_step = fold
    try:
        w = net._decoder_weights().struct
        assert bool(w.rnn_whh_frag) == fold and bool(w.rnn_gate_fold) == fold
        got = _decode(net)
        again = _decode(net)
    finally:
        net.fold_decoder_step = True
    assert torch.equal(got["predictions"].cpu(), T(g["predictions"]))           # copied (>= VT) and collapsed winners included:
    assert torch.equal(got["predictions"].cpu(), ref["predictions"])
    cls = g["classes"]
    assert int((got["predictions"] >= VT).sum()) == int(cls[0]) >= 1 and int(cls[1]) >= 1
    ok, fig = R.accept_decode(got, ref, chain, MAXLEN if fold else 0)
    print("acg_gru bound %s %s: %s" % (tag, "fast" if fold else "plain", fig))
    assert ok, fig
    assert float((got["attentions"].cpu() - R.pad_attn(g["attentions"], QL)).abs().max()) <= 1e-4
    masked = (torch.arange(QL).view(1, 1, QL) >= LENS.view(-1, 1, 1)).expand(-1, MAXLEN, -1)
    assert bool((got["attentions"].cpu()[masked] == 0).all())
    assert torch.equal(again["predictions"], got["predictions"]) and torch.equal(again["attentions"], got["attentions"])


def _collate(src, lens, tag):
    vocabs = AR.row_vocabs(src, lens)
    B = src.shape[0]
    toks = [[[AR.word(i) for i in src[b, :int(lens[b])].tolist()]] for b in range(B)]
    return dict(source_words=src.unsqueeze(1), source_lens=lens.unsqueeze(1), ids=["%s%d" % (tag, b) for b in range(B)], source_tokens=toks,
                target_tokens=[[["<s>", "a", "b", "</s>"]] for _ in range(B)], src_vocab=vocabs,
                src_map=[torch.tensor([vocabs[b][w] for w in toks[b][0]]) for b in range(B)])


@pytest.mark.parametrize("tag", R.ACG_CASES)
def test_predict_eager_then_graph_replay(cases, tag):
    r, c, g, ref, chain = cases[tag]
    ex = _collate(SRC, LENS, "a")
    r.predict_graph_min_calls = 2
    r.clear_predict_graphs()
    a = r.predict(ex)                                                   # eager
    b = r.predict(ex)                                                   # captured and replayed
    d = r.predict(ex)                                                   # replayed
    assert r._graphs is not None and r._graphs.captures == 1 and r._graphs.replays >= 2
    for o in (a, b, d):
        assert torch.equal(o["prediction_ids"].cpu(), T(g["predictions"]))
        assert torch.equal(o["attentions"], a["attentions"]) and o["predictions"] == a["predictions"]


# ---- train mode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,force", [(t, False) for t in R.ACG_CASES] + [("general", True)])
def test_copy_loss_and_gradients_against_fp64(tag, force):
    net, c, g = R.case("acg", tag, force_copy=force)
    net = net.to(DEV)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net.dec_dropout_p = 0.0
    net.train()
    loss = net(SRC.to(DEV), LENS.to(DEV), D["tw"].to(DEV), D["tlen"].to(DEV), D["ts"].to(DEV), D["maps"], D["al"])
    loss.backward()
    want = float(G["loss_force_copy"]) if force else float(g["loss"])
    print("acg_gru loss %s force_copy=%s: %.7f (reference %.7f)" % (tag, force, float(loss), want))
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    params = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    p = dict(params)
    p[R.S.EMB] = torch.cat([params[R.S.EMB][:1].detach(), params[R.S.EMB][1:]], 0)      # nn.Embedding(padding_idx=PAD): no gradient for the PAD row
    ref = R.acg_loss(p, c, SRC, LENS, D["tw"], D["ts"], D["idx"], D["al"], force_copy=force)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    for name, prm in net.named_parameters():
        gr = params[name].grad
        if "copy_attn.linear_out" in name:                              # in the state dict, in no value (rnn_decoder.py:83: only the alignment is used)
            assert gr is None and (prm.grad is None or float(prm.grad.abs().max()) == 0.0)
            continue
        assert prm.grad is not None, name
        err = (prm.grad.cpu().double() - gr).abs().max() / max(float(gr.abs().max()), 1e-5)
        print("acg_gru grad %s force_copy=%s %s: %.3g" % (tag, force, name, float(err)))
        assert float(err) < 1e-4, (name, float(err))


@pytest.mark.parametrize("fix", [True, False])
def test_recorded_update_losses(fix):
    r = _wrap("general", dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0, momentum=0,
              grad_clipping=10.0, fix_embeddings=fix)
    r.init_optimizer()
    batches = []
    for bi in range(2):
        d = R.acg_batch("train_b%d_" % bi)
        batches.append(dict(source_words=d["src"].unsqueeze(1), source_lens=d["lens"].unsqueeze(1), target_words=d["tw"].unsqueeze(1),
                            target_seq=d["ts"].unsqueeze(1), target_lens=d["tlen"].unsqueeze(1), src_map=d["maps"], alignment=d["als"]))
    losses = [float(r.update(batches[step % 2])) for step in range(3)]
    print("acg_gru update losses (fix_embeddings=%s): %s" % (fix, losses))
    np.testing.assert_allclose(losses, G["train_losses_" + ("fix" if fix else "free")], rtol=1e-4, atol=0)
    assert r.updates == 3
