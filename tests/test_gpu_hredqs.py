"""GPU (-m gpu): the HredQS mirror (csrc/hredqs.hip, recommender/hredqs.py, wrappers/recommender.py) against the reference's recorded decode,
encode states, loss and update losses (tests/golden/hredqs.npz, written by generate_hredqs.py) and against the fp64 restatement of
tests/hredqs_ref.py: every fixture case in both decode forms (exact tokens, the bound on the session states, the packs of the fast form,
bitwise repeatability), the two forms against each other, the C entry against nir_decode_greedy_plain_folded fed the same paired states,
B = 1, S = 1, max_len = 1, identity dictionaries, eager predict against graph replay and the text fields, and train mode (loss, every
gradient, recorded update losses, decode after the updates)."""
import numpy as np
import pytest
import torch

import hredqs_ref as R
from conftest import T, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = load_golden("hredqs")
MAXLEN, VT = int(G["max_len"]), int(G["tgt_vocab"])
SPECIAL = ["<blank>", "<unk>", "<s>", "</s>"]
TGT_DICT = [SPECIAL[i] if i < 4 else "w%d" % i for i in range(VT)]
SRC_DICT = {TGT_DICT[i]: int(s) for i, s in enumerate(G["tgt2src"])}        # src_dict[tgt_dict[i]] = tgt2src[i]
FORMS = ("fast", "plain")


def _wrap(tag, **kw):
    from context_attentive_ir_amd.wrappers import SessionRecommender
    net = R.case(tag)[0]
    r = SessionRecommender(R.case_args(tag, **kw), SRC_DICT, TGT_DICT, net.state_dict())
    r.cuda()
    r.network.eval()
    return r


@pytest.fixture(scope="module")
def cases():
    """every fixture case once: (wrapper on the GPU, cfg, golden arrays, fp64 decode, fp32 decode)"""
    out = {}
    for tag in R.CASES:
        net, c, g = R.case(tag)
        sd, lut = net.state_dict(), T(g["tgt2src"])
        out[tag] = (_wrap(tag), c, g, R.decode(sd, g["source_words"], g["source_lens"], MAXLEN, lut),
                    R.decode(sd, g["source_words"], g["source_lens"], MAXLEN, lut, torch.float32))
    return out


def _decode(net, src, lens, max_len=MAXLEN, dicts=True):
    """decode + encode -> dict(predictions, enc_h, enc_c)"""
    B, S, QL = src.shape
    out = net.decode(src.to(DEV), lens.to(DEV), max_len, SRC_DICT if dicts else None, TGT_DICT if dicts else None)
    assert set(out) == {"predictions"}                                     # there are no attentions
    h, c = net.encode(src.reshape(B * S, QL).to(DEV), lens.reshape(-1).to(DEV), B, S)
    return dict(predictions=out["predictions"], enc_h=h, enc_c=c)


class _form(object):
    """`with _form(net, "plain")`: the entry's plain form (net.fast_decode = False), restored on exit"""

    def __init__(self, net, form):
        self.net, self.fast = net, form == "fast"

    def __enter__(self):
        self.net.fast_decode = self.fast
        return self.net._decoder_weights().struct

    def __exit__(self, *exc):
        self.net.fast_decode = True
        return False


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tag", R.CASES)
def test_decode_matches_the_reference_and_the_fp64_bound(cases, tag, form):
    r, c, g, ref, chain = cases[tag]
    net = r.network
    src, lens = g["source_words"], g["source_lens"]
    B, S, QL = src.shape
    with _form(net, form) as w:
        # detinit weights are far inside the split range: the fast form has all three packs, the plain form none
        assert (bool(w.gen_frag), bool(w.rnn_whh_frag), bool(w.rnn_gate_fold)) == ((True,) * 3 if form == "fast" else (False,) * 3)
        got = _decode(net, src, lens)
        again = _decode(net, src, lens)
    assert got["predictions"].shape == (B, S, MAXLEN) and got["predictions"].dtype == torch.int64
    assert got["enc_h"].shape == got["enc_c"].shape == (1, S * B, c["nhid_session"])
    assert torch.equal(got["predictions"].cpu(), T(g["predictions"]))
    ok, fig = R.accept_decode(got, ref, chain, R.n_split(QL, S))
    print("hredqs bound %s %s: %s" % (tag, form, fig))
    assert ok, fig
    for k in ("enc_h", "enc_c"):
        assert float((got[k].cpu() - T(g[k])).abs().max()) <= 1e-4
        assert torch.equal(again[k], got[k])
    assert torch.equal(again["predictions"], got["predictions"])


@pytest.mark.parametrize("tag", R.CASES)
def test_fast_and_plain_forms_give_the_same_tokens(cases, tag):
    r, c, g, _, _ = cases[tag]
    net = r.network
    src, lens = g["source_words"].to(DEV), g["source_lens"].to(DEV)
    out = {}
    for form in FORMS:
        with _form(net, form):
            out[form] = net.decode(src, lens, MAXLEN, SRC_DICT, TGT_DICT)["predictions"]
    assert torch.equal(out["fast"], out["plain"])


@pytest.mark.parametrize("tag", R.CASES)
def test_c_entry_agrees_with_the_plain_folded_decoder_on_the_same_paired_states(cases, tag):
    from context_attentive_ir_amd import lib
    r, c, g, _, _ = cases[tag]
    net = r.network
    L = lib.load()
    src, lens = g["source_words"], g["source_lens"]
    B, S, QL = src.shape
    R_, H = B * S, c["nhid_session"]
    with torch.no_grad():
        hs, cs = net._session_steps(src.reshape(R_, QL).to(DEV), lens.reshape(-1).to(DEV), B, S)          # [B, S, H]
    w = net._decoder_weights()
    assert w.struct.gen_frag and w.struct.rnn_whh_frag and w.struct.rnn_gate_fold
    table = net.embedder.word_embeddings.table.detach().float().contiguous()
    lut = T(g["tgt2src"]).to(DEV)
    # the pairing on the host: decode row r starts from step r // B of session r % B
    idx = torch.tensor([(i % B) * S + i // B for i in range(R_)], device=DEV)
    ph, pc = hs.reshape(R_, H)[idx].contiguous(), cs.reshape(R_, H)[idx].contiguous()
    assert torch.equal(ph, hs.transpose(0, 1).reshape(R_, H))
    k = w.keep
    base = torch.full((R_, MAXLEN), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(L.nir_decode_greedy_plain_workspace_bytes(R_, H, VT), dtype=torch.uint8, device=DEV)
    lib.check(L.nir_decode_greedy_plain_folded(lib.ptr(ph), lib.ptr(pc), R_, H, lib.ptr(table), table.shape[0], table.shape[1], lib.ptr(k["rnn_wih"]),
                                               lib.ptr(k["rnn_whh"]), lib.ptr(k["rnn_bih"]), lib.ptr(k["rnn_bhh"]), lib.ptr(k["gen_w"]),
                                               lib.ptr(k["gen_b"]), VT, lib.ptr(lut), 2, MAXLEN, lib.ptr(k["rnn_gate_fold"]),
                                               lib.ptr(k["rnn_whh_frag"]), lib.ptr(ws), ws.numel(), lib.ptr(base), lib.stream()),
              "nir_decode_greedy_plain_folded")
    got = torch.full((B, S, MAXLEN), -7, dtype=torch.int64, device=DEV)
    ws2 = torch.empty(L.nir_hredqs_decode_workspace_bytes(B, S, MAXLEN, w.ref()), dtype=torch.uint8, device=DEV)
    lib.check(L.nir_hredqs_decode_greedy(lib.ptr(hs), lib.ptr(cs), B, S, lib.ptr(table), table.shape[0], table.shape[1], lib.ptr(lut), 2, MAXLEN,
                                         w.ref(), lib.ptr(ws2), ws2.numel(), lib.ptr(got), lib.stream()), "nir_hredqs_decode_greedy")
    torch.cuda.synchronize()
    assert torch.equal(got.view(R_, MAXLEN), base)
    assert torch.equal(got.cpu(), T(g["predictions"]))


def test_entry_argument_checks_and_empty_shapes(cases):
    from context_attentive_ir_amd import lib
    r, c, g, _, _ = cases["h64"]
    net = r.network
    L = lib.load()
    B, S, H = 3, 4, c["nhid_session"]
    w = net._decoder_weights()
    table = net.embedder.word_embeddings.table.detach().float().contiguous()
    hs, cs = torch.zeros(B, S, H, device=DEV), torch.zeros(B, S, H, device=DEV)
    need = L.nir_hredqs_decode_workspace_bytes(B, S, MAXLEN, w.ref())
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(Bx=B, Sx=S, V=table.shape[0], E=table.shape[1], bos=2, max_len=MAXLEN, ws_bytes=need, ref=None):
        pred = torch.full((B, S, MAXLEN), -7, dtype=torch.int64, device=DEV)
        rc = L.nir_hredqs_decode_greedy(lib.ptr(hs), lib.ptr(cs), Bx, Sx, lib.ptr(table), V, E, None, bos, max_len,
                                        ref if ref is not None else w.ref(), lib.ptr(ws), ws_bytes, lib.ptr(pred), lib.stream())
        torch.cuda.synchronize()
        return rc, bool((pred == -7).all())
    assert call(bos=table.shape[0]) == (-1, True)
    assert call(E=table.shape[1] - 2) == (-1, True)
    assert call(Bx=-1) == (-1, True)
    assert call(ws_bytes=need - 256) == (-3, True)
    half = type(w.struct).from_buffer_copy(w.struct)
    half.rnn_gate_fold = None
    assert call(ref=lib.C.byref(half)) == (-1, True)
    assert call(Bx=0) == (0, True) and call(Sx=0) == (0, True) and call(max_len=0) == (0, True)          # nothing enqueued
    rc, untouched = call()
    assert rc == 0 and not untouched


# ---- edge and option cases -------------------------------------------------------------------------------------------------------------
def _against_restatement(net, src, lens, max_len, lut, tag):
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    ref = R.decode(sd, src, lens, max_len, lut)
    chain = R.decode(sd, src, lens, max_len, lut, torch.float32)
    assert float(ref["gaps"].min()) >= 1e-4, "the case's own logit gaps are too small to compare tokens: %s" % ref["gaps"].min()
    out = {}
    for form in FORMS:
        with _form(net, form):
            out[form] = _decode(net, src, lens, max_len, dicts=lut is not None)
        ok, fig = R.accept_decode(out[form], ref, chain, R.n_split(src.shape[2], src.shape[1]))
        print("hredqs bound %s %s: %s" % (tag, form, fig))
        assert ok, fig
    return out["fast"]


# (h96 and h1024: every edge shape below keeps its float64 logit gaps >= 1e-3 there; H = 96 is no multiple of 64, H = 1024 the narrow row tile)
@pytest.mark.parametrize("tag", ["h96", "h1024"])
def test_single_session_single_query_single_step_and_identity_dictionaries(cases, tag):
    r, c, g, _, _ = cases[tag]
    src, lens, lut = g["source_words"], g["source_lens"], T(g["tgt2src"])
    _against_restatement(r.network, src[1:2].contiguous(), lens[1:2].contiguous(), MAXLEN, lut, tag + " B=1")
    _against_restatement(r.network, src[:, 2:3].contiguous(), lens[:, 2:3].contiguous(), MAXLEN, lut, tag + " S=1")
    got = _against_restatement(r.network, src, lens, 1, lut, tag + " max_len=1")
    assert got["predictions"].shape == (src.shape[0], src.shape[1], 1)
    # without dictionaries the predicted target id is fed back as it is (V_tgt == V_src here)
    ident = _against_restatement(r.network, src, lens, MAXLEN, None, tag + " identity")
    assert not torch.equal(ident["predictions"].cpu(), T(g["predictions"]))          # the permuted src_dict matters from step 2 on
    empty = r.network.decode(src[:0].to(DEV), lens[:0].to(DEV), MAXLEN, SRC_DICT, TGT_DICT)["predictions"]
    assert empty.shape == (0, src.shape[1], MAXLEN)


@pytest.mark.parametrize("tag", ["h64", "h1024"])
def test_predict_eager_then_graph_replay(cases, tag):
    r, c, g, _, _ = cases[tag]
    r.predict_graph_min_calls = 2
    r.clear_predict_graphs()
    ex = dict(source_words=g["source_words"], source_lens=g["source_lens"])
    a = r.predict(ex)                                                   # eager
    b = r.predict(ex)                                                   # captured and replayed
    d = r.predict(ex)                                                   # replayed
    assert r._graphs is not None and r._graphs.captures == 1 and r._graphs.replays >= 2
    for o in (a, b, d):
        assert set(o) == {"prediction_ids"}
        assert o["prediction_ids"].shape == (c["B"], c["S"], MAXLEN)
        assert torch.equal(o["prediction_ids"].cpu(), T(g["predictions"]))


def test_predict_returns_the_references_text_fields(cases):
    r, c, g, _, _ = cases["h64"]
    B, S = c["B"], c["S"]
    lens = g["source_lens"]
    toks = [[["<s>"] + ["s%d_%d_%d" % (b, s, j) for j in range(int(lens[b, s]))] + ["</s>"] for s in range(S)] for b in range(B)]
    tgts = [[["<s>", "t%d_%d" % (b, s), "x", "</s>"] for s in range(S)] for b in range(B)]
    ex = dict(source_words=g["source_words"], source_lens=lens, ids=["q%d_" % b for b in range(B)], source_tokens=toks, target_tokens=tgts,
              src_vocab=None, session_len=S, batch_size=B)
    out = r.predict(ex)
    assert out["ex_ids"] == ["q%d_%d" % (b, s) for s in range(S) for b in range(B)]
    assert out["targets"] == [["t%d_%d x" % (b, s)] for s in range(S) for b in range(B)]
    assert out["src_sequences"] == [" ".join(" ".join(q[1:-1]) for q in toks[b][:s + 1]) for s in range(S) for b in range(B)]
    ids = g["predictions"]
    want = []
    for s in range(S):
        for b in range(B):
            sent = []
            for wd in ids[b, s].tolist():
                if wd == 2:
                    continue
                if wd == 3:
                    break
                sent.append(TGT_DICT[wd])
            want.append(" ".join(sent or ["0"]))
    assert out["predictions"] == want and len(want) == B * S
    assert torch.equal(out["prediction_ids"].cpu(), T(ids))


# ---- train mode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", R.CASES)
def test_loss_and_gradients_against_fp64(tag):
    net, c, g = R.case(tag)
    net = net.to(DEV)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net.dec_dropout_p = 0.0
    net.train()
    src, lens, tw, ts, tl = (g[k] for k in ("source_words", "source_lens", "target_words", "target_seq", "target_lens"))
    loss = net(src.to(DEV), lens.to(DEV), tw.to(DEV), tl.to(DEV), ts.to(DEV), None, None)
    loss.backward()
    print("hredqs loss %s: %.8g (recorded %.8g)" % (tag, float(loss), float(g["loss"])))
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    params = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    p = dict(params)
    p[R.EMB] = torch.cat([params[R.EMB][:1].detach(), params[R.EMB][1:]], 0)          # nn.Embedding(padding_idx=PAD): no gradient for the PAD row
    ref = R.loss(p, src, lens, tw, ts)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    for name, prm in net.named_parameters():
        gr = params[name].grad
        assert prm.grad is not None, name
        err = (prm.grad.cpu().double() - gr).abs().max() / max(float(gr.abs().max()), 1e-5)
        print("hredqs grad %s %s: %.3g" % (tag, name, float(err)))
        assert float(err) < 1e-4, (name, float(err))


@pytest.mark.parametrize("fix", [True, False])
def test_recorded_update_losses_and_decode_after_them(fix):
    from context_attentive_ir_amd.wrappers import SessionRecommender
    net, c, g = R.case("h64")
    r = SessionRecommender(R.case_args("h64", dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0,
                                       momentum=0, grad_clipping=10.0, fix_embeddings=fix), list(range(int(G["vocab"]))), list(range(VT)),
                           net.state_dict())
    r.cuda()
    r.init_optimizer()
    # one decode BEFORE the updates, so that the packs of the old weights exist: a stale pack would show below
    r.network.eval()
    r.network.decode(g["source_words"].to(DEV), g["source_lens"].to(DEV), MAXLEN, None, None)
    batches = [{k: T(G["train_b%d_%s" % (bi, k)]) for k in ("source_words", "source_lens", "target_words", "target_seq", "target_lens")}
               for bi in range(2)]
    losses = [float(r.update(batches[step % 2])) for step in range(3)]
    print("hredqs update losses (fix_embeddings=%s): %s" % (fix, losses))
    np.testing.assert_allclose(losses, G["train_losses_" + ("fix" if fix else "free")], rtol=1e-4, atol=0)
    assert r.updates == 3
    assert r.network.embedder.word_embeddings.table.requires_grad == (not fix)
    r.network.eval()
    _against_restatement(r.network, g["source_words"], g["source_lens"], MAXLEN, None, "after 3 updates fix=%s" % fix)
