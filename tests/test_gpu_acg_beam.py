"""GPU (-m gpu): beam search for ACG and ACGGRU (csrc/beam.hip: acg_beam_row_kernel, acg_beam_select_kernel; ACG.decode_beam,
CopyRecommender.predict_nbest) against the float64 restatement of tests/acg_beam_ref.py, which forms the full collapsed distribution of every
row, on the fixtures of tests/golden/acg_beam_seeds.json: tokens, back-pointers and lengths exactly, scores and attentions inside their
bounds; the fused / plain generator forms and the folded / plain step forms against each other; bitwise repeatability; eager against graph
replay over two batches of one shape with different maps; W = 1 against the greedy decode on the unmodified fixtures; the n-best text."""
import pytest
import torch

import acg_beam_ref as R
import acg_ref as AR
import gru_dec_ref as GR
from conftest import T

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = R.batch()
SRC, LENS = D["src"], D["lens"]
QL, VT = SRC.shape[1], len(D["tgt_dict"])
CASE_W = [(k, t, W) for k, t in R.CASES for W in R.widths(k, t)]


def _wrap(kind, tag, net, max_len):
    from context_attentive_ir_amd.wrappers import CopyRecommender
    args = GR.case_args("acg", tag, max_query_len=max_len) if kind == "gru" else AR.case_args(tag, max_query_len=max_len)
    r = CopyRecommender(args, D["src_dict"], D["tgt_dict"], net.state_dict())
    r.cuda()
    r.network.eval()
    return r


@pytest.fixture(scope="module")
def cases():
    """every (case, W) once: (wrapper on the GPU, fp64 decode, fp32 decode forced along the fp64 choices)"""
    out = {}
    for kind, tag, W in CASE_W:
        net, c, cell = R.case(kind, tag, W)
        sd = net.state_dict()
        args = (sd, c, cell, SRC, LENS, R.max_len(W), W, D["idx"], D["e2t"], D["e2s"])
        ref = R.decode(*args)
        chain = R.decode(*args, dtype=torch.float32, force=(ref["backptr"], ref["tokens"]))
        out[kind, tag, W] = (_wrap(kind, tag, net, R.max_len(W)), ref, chain)
    return out


def _decode(net, W, max_len=None, **kw):
    return net.decode_beam(SRC.to(DEV), LENS.to(DEV), R.max_len(W) if max_len is None else max_len, W, D["src_dict"], D["tgt_dict"],
                           src_map_idx=D["idx"], ext2tgt=D["e2t"], ext2src=D["e2s"], return_backptr=True, **kw)


def _n_split(net, max_len):
    """split products on the path of a score: one recurrent (fp16-term step) and one generator product (fused top-k) per step"""
    w = net._decoder_weights().struct
    return max_len * (int(bool(w.rnn_whh_frag)) + int(bool(w.gen_frag) and net.fuse_generator_topk))


@pytest.mark.parametrize("kind,tag,W", CASE_W)
def test_beam_decode_matches_the_fp64_restatement(cases, kind, tag, W):
    r, ref, chain = cases[kind, tag, W]
    net, L = r.network, R.max_len(W)
    got = _decode(net, W)
    B = SRC.shape[0]
    assert got["predictions"].shape == (B, W, L) and got["predictions"].dtype == torch.int64
    assert got["scores"].shape == (B, W) and got["lengths"].shape == (B, W) and got["attentions"].shape == (B, W, L, QL)
    w = net._decoder_weights().struct
    assert w.gen_frag and w.rnn_whh_frag and w.rnn_gate_fold                 # the fast forms ran
    ok, fig = R.accept_decode(got, ref, chain, _n_split(net, L))
    print("acg beam bound %s %s W=%d: scores %s attentions %s" % (kind, tag, W, fig["scores"], fig["attentions"]))
    assert ok, fig
    sc = got["scores"].cpu()
    assert bool((sc[:, :-1] >= sc[:, 1:]).all())                             # best beam first
    if W > 1:
        assert bool((got["predictions"] >= VT).any())                        # a copied word among the suggestions
    masked = (torch.arange(QL).view(1, 1, 1, QL) >= LENS.view(-1, 1, 1, 1)).expand(-1, W, L, -1)
    assert bool((got["attentions"].cpu()[masked] == 0).all())
    again = _decode(net, W)
    for k in ("predictions", "scores", "lengths", "attentions", "backptr"):
        assert torch.equal(again[k], got[k]), k                              # the same bits


@pytest.mark.parametrize("kind,tag", [("lstm", "dot"), ("lstm", "own"), ("lstm", "wide"), ("gru", "general")])
def test_generator_and_step_forms_agree_in_every_token(cases, kind, tag):
    r, ref, chain = cases[kind, tag, 4]
    net = r.network
    try:
        for fold, fuse in ((True, False), (False, True), (False, False)):
            net.fold_decoder_step, net.fuse_generator_topk = fold, fuse
            assert bool(net._decoder_weights().struct.rnn_whh_frag) == fold
            got = _decode(net, 4)
            ok, fig = R.accept_decode(got, ref, chain, _n_split(net, R.max_len(4)))
            print("acg beam bound %s %s fold=%s fuse=%s: scores %s" % (kind, tag, fold, fuse, fig["scores"]))
            assert ok, fig
    finally:
        net.fold_decoder_step = net.fuse_generator_topk = True


def _collate(src, lens, tag):
    vocabs = AR.row_vocabs(src, lens)
    B = src.shape[0]
    toks = [[[AR.word(i) for i in src[b, :int(lens[b])].tolist()]] for b in range(B)]
    return dict(source_words=src.unsqueeze(1), source_lens=lens.unsqueeze(1), ids=["%s%d" % (tag, b) for b in range(B)], source_tokens=toks,
                target_tokens=[[["<s>", "a", "b", "</s>"]] for _ in range(B)], src_vocab=vocabs,
                src_map=[torch.tensor([vocabs[b][w] for w in toks[b][0]]) for b in range(B)])


def _other_batch():
    """the fixture's shape with other words and the repeat moved (as many distinct words per row, so the same CV): all three maps differ"""
    src = torch.where(SRC >= 4, (SRC - 4 + 17) % 256 + 4, SRC)
    r = int(LENS.argmax())
    src[r, 2] = next(i for i in range(4, 260) if i not in src[r].tolist())
    src[r, 3] = src[r, 1]
    return src


@pytest.mark.parametrize("kind,tag", [("lstm", "general"), ("gru", "general")])
def test_predict_nbest_eager_then_graph_replay_with_two_batches_of_one_shape(cases, kind, tag):
    r, ref, chain = cases[kind, tag, 4]
    exA, exB = _collate(SRC, LENS, "a"), _collate(_other_batch(), LENS, "b")
    fA, fB = r._copy_fields(exA), r._copy_fields(exB)
    assert all(fA[k].shape == fB[k].shape and not torch.equal(fA[k], fB[k]) for k in r._FIELDS[2:])
    r.args.predict_graphs = False
    eA, eB = r.predict_nbest(exA, 4), r.predict_nbest(exB, 4)             # eager
    r.args.predict_graphs = True
    r.predict_graph_min_calls = 2
    r.clear_predict_graphs()
    a1 = r.predict_nbest(exA, 4)                                          # first sighting of the shape: eager
    b1 = r.predict_nbest(exB, 4)                                          # captured over B's maps, replayed
    a2 = r.predict_nbest(exA, 4)                                          # replayed: must read A's maps
    b2 = r.predict_nbest(exB, 4)
    assert r._graphs is not None and r._graphs.captures == 1 and r._graphs.replays >= 3
    assert torch.equal(eA["prediction_ids"].cpu(), ref["predictions"]) and torch.equal(eA["lengths"].cpu(), ref["lengths"])
    assert not torch.equal(eA["prediction_ids"], eB["prediction_ids"])
    for got, want in ((a1, eA), (a2, eA), (b1, eB), (b2, eB)):
        assert set(got) >= {"prediction_ids", "scores", "lengths", "attentions", "predictions"}
        for k in ("prediction_ids", "scores", "lengths", "attentions"):
            assert torch.equal(got[k], want[k]), k
        assert got["predictions"] == want["predictions"]


def test_predict_nbest_returns_n_best_text_with_a_copied_word(cases):
    r, ref, chain = cases["lstm", "general", 4]
    ex = _collate(SRC, LENS, "q")
    out = r.predict_nbest(ex, 4)
    B = SRC.shape[0]
    assert out["ex_ids"] == ex["ids"] and out["targets"] == [["a b"]] * B
    copied = 0
    for b in range(B):
        assert len(out["predictions"][b]) == 4
        for k in range(4):
            want = []
            for wd in ref["predictions"][b, k].tolist():                     # tens2sen with the rows' dictionaries
                if wd == 2:
                    continue
                if wd == 3:
                    break
                want.append(D["tgt_dict"][wd] if wd < VT else ex["src_vocab"][b][wd - VT])
                copied += wd >= VT
            want = want or ["0"]
            att = out["attentions"][b, k].cpu()
            want = [ex["source_tokens"][b][0][int(att[i].argmax())] if w == "<unk>" else w for i, w in enumerate(want)]
            assert out["predictions"][b][k] == " ".join(want)
    assert copied >= 1


@pytest.mark.parametrize("kind,tag", [("lstm", t) for t in AR.CASES] + [("gru", t) for t in GR.ACG_CASES])
def test_width_one_equals_the_greedy_decode_token_for_token(kind, tag):
    net, c, g = AR.case(tag) if kind == "lstm" else GR.case("acg", tag)        # the unmodified greedy fixture
    max_len = int(AR.golden()["max_len"])
    net = _wrap(kind, tag, net, max_len).network
    greedy = net.decode(SRC.to(DEV), LENS.to(DEV), max_len, D["src_dict"], D["tgt_dict"], src_map_idx=D["idx"], ext2tgt=D["e2t"], ext2src=D["e2s"])
    beam = _decode(net, 1, max_len=max_len)
    assert torch.equal(greedy["predictions"].cpu(), T(g["predictions"]))
    assert torch.equal(beam["predictions"][:, 0], greedy["predictions"])
    assert torch.equal(beam["attentions"][:, 0], greedy["attentions"])       # the same kernels on the same rows: the same bits
    assert bool((beam["backptr"] == 0).all())
