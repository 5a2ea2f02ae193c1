"""GPU (-m gpu): the ACG mirror (csrc/acg.hip, recommender/acg.py, wrappers.CopyRecommender) against the reference's recorded decode,
losses and update losses (tests/golden/acg.npz, written by generate_acg.py) and against the fp64 restatement of tests/acg_ref.py: every
fixture case on both forms of the generator statistics (fused, plain), exact tokens, attentions, exact zeros at masked positions, bitwise
repeatability, the reference's own argument forms, train mode (loss, every gradient, force_copy, recorded update losses), eager predict
against graph replay over two batches of one shape with different maps, and the text tail."""
import numpy as np
import pytest
import torch

import acg_ref as R
from conftest import T

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = R.golden()
D = R.batch_inputs()
SRC, LENS = D["src"], D["lens"]
QL, MAXLEN, VT = SRC.shape[1], int(G["max_len"]), int(G["tgt_vocab"])
E2T, E2S = R.index_tensors(D)


def _wrap(tag, **kw):
    from context_attentive_ir_amd.wrappers import CopyRecommender
    net = R.case(tag)[0]
    r = CopyRecommender(R.case_args(tag, **kw), D["src_dict"], D["tgt_dict"], net.state_dict())
    r.cuda()
    r.network.eval()
    return r


@pytest.fixture(scope="module")
def cases():
    """every fixture case once: (wrapper on the GPU, cfg, golden arrays, fp64 decode)"""
    out = {}
    for tag in R.CASES:
        net, c, g = R.case(tag)
        out[tag] = (_wrap(tag), c, g, R.decode(net.state_dict(), c, SRC, LENS, MAXLEN, D["idx"], E2T, E2S))
    return out


def _decode(net, **kw):
    return net.decode(SRC.to(DEV), LENS.to(DEV), MAXLEN, D["src_dict"], D["tgt_dict"], src_map_idx=D["idx"], ext2tgt=E2T, ext2src=E2S, **kw)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("tag", R.CASES)
def test_decode_matches_the_reference(cases, tag, fused):
    r, c, g, ref = cases[tag]
    net = r.network
    net.fuse_generator_argmax = fused
    try:
        assert bool(net._decoder_weights().struct.gen_frag) == fused
        got = _decode(net)
        again = _decode(net)
    finally:
        net.fuse_generator_argmax = True
    assert got["predictions"].shape == (SRC.shape[0], MAXLEN) and got["predictions"].dtype == torch.int64
    assert torch.equal(got["predictions"].cpu(), T(g["predictions"]))
    assert torch.equal(got["predictions"].cpu(), ref["predictions"])
    err = float((got["attentions"].cpu() - R.pad_attn(g["attentions"], QL)).abs().max())
    print("acg attentions %s %s: max |diff| %.3g" % (tag, "fused" if fused else "plain", err))
    assert err <= 1e-4
    masked = (torch.arange(QL).view(1, 1, QL) >= LENS.view(-1, 1, 1)).expand(-1, MAXLEN, -1)
    assert bool((got["attentions"].cpu()[masked] == 0).all())
    assert torch.equal(again["predictions"], got["predictions"]) and torch.equal(again["attentions"], got["attentions"])


def test_decode_takes_the_references_arguments(cases):
    r, c, g, ref = cases["general"]
    blank, fill = R.collapse_copy_scores(D["tgt_dict"], D["vocabs"])
    for src_map in (D["maps"], R.make_src_map(D["maps"])):
        got = r.network.decode(source_rep=SRC.to(DEV), source_len=LENS.to(DEV), max_len=MAXLEN, src_dict=D["src_dict"], tgt_dict=D["tgt_dict"],
                               src_map=src_map, alignment=None, blank=blank, fill=fill, source_vocabs=D["vocabs"])
        assert torch.equal(got["predictions"].cpu(), T(g["predictions"]))


# ---- train mode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,force", [(t, False) for t in R.CASES] + [("general", True)])
def test_loss_and_gradients_against_fp64(tag, force):
    net, c, g = R.case(tag, force_copy=force)
    net = net.to(DEV)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net.dec_dropout_p = 0.0
    net.train()
    loss = net(SRC.to(DEV), LENS.to(DEV), D["tw"].to(DEV), D["tlen"].to(DEV), D["ts"].to(DEV), D["maps"], D["al"])
    loss.backward()
    want = float(G["loss_force_copy"]) if force else float(g["loss"])
    print("acg loss %s force_copy=%s: %.7f (reference %.7f)" % (tag, force, float(loss), want))
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    params = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    p = dict(params)
    p[R.S.EMB] = torch.cat([params[R.S.EMB][:1].detach(), params[R.S.EMB][1:]], 0)      # nn.Embedding(padding_idx=PAD): no gradient for the PAD row
    ref = R.loss(p, c, SRC, LENS, D["tw"], D["ts"], D["idx"], D["al"], force_copy=force)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    for name, prm in net.named_parameters():
        gr = params[name].grad
        if "copy_attn.linear_out" in name:                              # in the state dict, in no value (rnn_decoder.py:83: only the alignment is used)
            assert gr is None and (prm.grad is None or float(prm.grad.abs().max()) == 0.0)
            continue
        assert prm.grad is not None, name
        err = (prm.grad.cpu().double() - gr).abs().max() / max(float(gr.abs().max()), 1e-5)
        print("acg grad %s force_copy=%s %s: %.3g" % (tag, force, name, float(err)))
        assert float(err) < 1e-4, (name, float(err))


def _train_batches():
    out = []
    for bi in range(2):
        d = R.batch_inputs("train_b%d_" % bi)
        out.append(dict(source_words=d["src"].unsqueeze(1), source_lens=d["lens"].unsqueeze(1), target_words=d["tw"].unsqueeze(1),
                        target_seq=d["ts"].unsqueeze(1), target_lens=d["tlen"].unsqueeze(1), src_map=d["maps"], alignment=d["als"]))
    return out


@pytest.mark.parametrize("fix", [True, False])
def test_recorded_update_losses(fix):
    r = _wrap("general", dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0, momentum=0,
              grad_clipping=10.0, fix_embeddings=fix)
    r.init_optimizer()
    batches = _train_batches()
    losses = [float(r.update(batches[step % 2])) for step in range(3)]
    print("acg update losses (fix_embeddings=%s): %s" % (fix, losses))
    np.testing.assert_allclose(losses, G["train_losses_" + ("fix" if fix else "free")], rtol=1e-4, atol=0)
    assert r.updates == 3
    # decode at the new weights: a stale pack would miss the restatement on the network's own state dict
    r.network.eval()
    sd = {k: v.cpu() for k, v in r.network.state_dict().items()}
    ref = R.decode(sd, R.case_cfg("general"), SRC, LENS, MAXLEN, D["idx"], E2T, E2S)
    got = _decode(r.network)
    compared = 0
    for b in range(SRC.shape[0]):                                         # the updated weights have gaps of their own: a row is compared up to
        close = (ref["gaps"][b] < 1e-3).nonzero()                         # its first step below the fixture's bar (1e-3, ten times the parity bar)
        n = int(close[0]) if len(close) else MAXLEN
        assert torch.equal(got["predictions"].cpu()[b, :n], ref["predictions"][b, :n])
        compared += n
    assert compared >= MAXLEN


# ---- the wrapper's predict -------------------------------------------------------------------------------------------------------------
def _collate(src, lens, tag):
    vocabs = R.row_vocabs(src, lens)
    B = src.shape[0]
    toks = [[[R.word(i) for i in src[b, :int(lens[b])].tolist()]] for b in range(B)]
    return dict(source_words=src.unsqueeze(1), source_lens=lens.unsqueeze(1), ids=["%s%d" % (tag, b) for b in range(B)], source_tokens=toks,
                target_tokens=[[["<s>", "a", "b", "</s>"]] for _ in range(B)], src_vocab=vocabs,
                src_map=[torch.tensor([vocabs[b][w] for w in toks[b][0]]) for b in range(B)])


def _other_batch():
    """the fixture's shape with other words and the repeat moved (as many distinct words per row, so the same CV): all three maps differ"""
    src = torch.where(SRC >= 4, (SRC - 4 + 17) % 256 + 4, SRC)
    r = int(LENS.argmax())
    src[r, 2] = next(i for i in range(4, 260) if i not in src[r].tolist())      # positions 0 and 2 held the repeated word
    src[r, 3] = src[r, 1]
    return src


def test_predict_eager_then_graph_replay_with_two_batches_of_one_shape(cases):
    r, c, g, ref = cases["general"]
    exA, exB = _collate(SRC, LENS, "a"), _collate(_other_batch(), LENS, "b")
    fA, fB = r._copy_fields(exA), r._copy_fields(exB)
    assert all(fA[k].shape == fB[k].shape and not torch.equal(fA[k], fB[k]) for k in r._FIELDS[2:])
    r.args.predict_graphs = False
    eA, eB = r.predict(exA), r.predict(exB)                               # eager
    r.args.predict_graphs = True
    r.predict_graph_min_calls = 2
    r.clear_predict_graphs()
    a1 = r.predict(exA)                                                   # first sighting of the shape: eager
    b1 = r.predict(exB)                                                   # captured over B's maps, replayed
    a2 = r.predict(exA)                                                   # replayed: must read A's maps
    b2 = r.predict(exB)
    assert r._graphs is not None and r._graphs.captures == 1 and r._graphs.replays >= 3
    assert torch.equal(eA["prediction_ids"].cpu(), T(g["predictions"]))
    assert not torch.equal(eA["prediction_ids"], eB["prediction_ids"])
    for o in (a1, a2):
        assert torch.equal(o["prediction_ids"], eA["prediction_ids"]) and torch.equal(o["attentions"], eA["attentions"])
        assert o["predictions"] == eA["predictions"]
    for o in (b1, b2):
        assert torch.equal(o["prediction_ids"], eB["prediction_ids"]) and torch.equal(o["attentions"], eB["attentions"])
        assert o["predictions"] == eB["predictions"]


def test_predict_returns_the_references_text_fields(cases):
    r, c, g, ref = cases["general"]
    ex = _collate(SRC, LENS, "q")
    out = r.predict(ex)
    B = SRC.shape[0]
    assert out["ex_ids"] == ex["ids"] and out["targets"] == [["a b"]] * B
    assert out["src_sequences"] == [[" ".join(t[0][1:-1])] for t in ex["source_tokens"]]
    ids = g["predictions"]
    copied = 0
    for b in range(B):
        want = []
        for wd in ids[b].tolist():                                        # tens2sen (utils/misc.py:36-62) with the rows' dictionaries
            if wd == 2:
                continue
            if wd == 3:
                break
            want.append(D["tgt_dict"][wd] if wd < VT else ex["src_vocab"][b][wd - VT])
            copied += wd >= VT
        want = want or ["0"]
        att = out["attentions"][b].cpu()
        want = [ex["source_tokens"][b][0][int(att[i].argmax())] if w == "<unk>" else w for i, w in enumerate(want)]     # replace_unknown
        assert out["predictions"][b] == " ".join(want)
    assert copied >= 1
