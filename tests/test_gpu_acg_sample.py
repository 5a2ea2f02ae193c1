"""GPU (-m gpu): sampling decode for ACG and ACGGRU (csrc/sample.hip: sample_gen_kernel<.., PAD>, acg_sample_row_kernel, the top-k form on
acg_beam_row_kernel's lists; ACG.sample_extended, CopyRecommender.sample_extended) against the float64 restatement of tests/acg_sample_ref.py,
which forms the full collapsed distribution of every row, on the six acg.npz cases with the seeds of acg_sample_ref.SEEDS: tokens and lengths
exactly, scores, token_logprobs and attentions inside their bounds; the fused and plain generator forms against each other; bitwise
repeatability; top_k = 1 against the greedy decode; the round trip through score_extended; the wrapper's text and seed."""
import pytest
import torch

import acg_ref as AR
import acg_sample_ref as R
import acg_score_ref as SC
import gru_dec_ref as GR
from conftest import T, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = R.batch()
SRC, LENS = D["src"], D["lens"]
QL, VT = SRC.shape[1], len(D["tgt_dict"])
MAPS = dict(src_map_idx=D["idx"], ext2tgt=D["e2t"], ext2src=D["e2s"])
CASE_SET = [(k, t, i) for k, t in R.CASES for i in range(len(R.SETTINGS))]


def _wrap(kind, tag, net, max_len=R.MAXLEN):
    from context_attentive_ir_amd.wrappers import CopyRecommender
    args = GR.case_args("acg", tag, max_query_len=max_len) if kind == "gru" else AR.case_args(tag, max_query_len=max_len)
    r = CopyRecommender(args, D["src_dict"], D["tgt_dict"], net.state_dict())
    r.cuda()
    r.network.eval()
    return r


@pytest.fixture(scope="module")
def nets():
    """every case once: (wrapper on the GPU, state dict, cfg, cell)"""
    out = {}
    for kind, tag in R.CASES:
        net, c, cell = R.case(kind, tag)
        out[kind, tag] = (_wrap(kind, tag, net), net.state_dict(), c, cell)
    return out


@pytest.fixture(scope="module")
def refs(nets):
    """(case, setting) -> (fp64 decode, fp32 decode forced along the fp64 tokens), computed once"""
    out = {}
    for kind, tag, i in CASE_SET:
        _, sd, c, cell = nets[kind, tag]
        tau, top_k = R.SETTINGS[i]
        a = (sd, c, cell, SRC, LENS, R.MAXLEN, R.N, R.SEEDS["%s_%s" % (kind, tag)][i], D["idx"], D["e2t"], D["e2s"], tau, top_k)
        ref = R.decode(*a)
        out[kind, tag, i] = (ref, R.decode(*a, dtype=torch.float32, force=ref["tokens"]))
    return out


@pytest.fixture(scope="module")
def worst():
    w = {"scores": float("-inf"), "token_logprobs": float("-inf")}
    yield w
    print("acg sample models: largest ratios %s" % {k: round(v, 3) for k, v in w.items()})


def _sample(net, seed, tau, top_k, max_len=R.MAXLEN, N=R.N, src=SRC, lens=LENS, maps=MAPS):
    return net.sample_extended(src.to(DEV), lens.to(DEV), max_len, N, tau, top_k, seed, D["src_dict"], D["tgt_dict"], **maps)


def _n_split(net, top_k, max_len=R.MAXLEN):
    """split products on the path of a score: one recurrent (fp16-term step) and one generator product (fused form) per step"""
    w = net._decoder_weights().struct
    fused = net.fuse_generator_topk if top_k > 0 else net.fuse_generator_argmax
    return max_len * (int(bool(w.rnn_whh_frag)) + int(bool(w.gen_frag) and fused))


@pytest.mark.parametrize("kind,tag,i", CASE_SET)
def test_samples_match_the_fp64_restatement_fused_and_plain(nets, refs, worst, kind, tag, i):
    net = nets[kind, tag][0].network
    ref, chain = refs[kind, tag, i]
    tau, top_k = R.SETTINGS[i]
    seed = R.SEEDS["%s_%s" % (kind, tag)][i]
    B = SRC.shape[0]
    outs = {}
    try:
        for fuse in (True, False):
            net.fuse_generator_argmax = net.fuse_generator_topk = fuse
            assert bool(net._decoder_weights().struct.gen_frag) == fuse                 # the form that was asked for runs
            got = _sample(net, seed, tau, top_k)
            assert got["predictions"].shape == (B, R.N, R.MAXLEN) and got["predictions"].dtype == torch.int64
            assert got["token_logprobs"].shape == (B, R.N, R.MAXLEN) and got["attentions"].shape == (B, R.N, R.MAXLEN, QL)
            ok, fig = R.accept_decode(got, ref, chain, _n_split(net, top_k))
            for k in worst:
                worst[k] = max(worst[k], fig[k]["ratio"])                               # what MARGIN is derived from
            print("acg sample %s %s tau=%g top_k=%d fused=%s: scores %s token_logprobs %s" % (kind, tag, tau, top_k, fuse, fig["scores"],
                                                                                             fig["token_logprobs"]))
            assert ok, fig
            assert bool((got["predictions"] >= 0).all()) and bool((got["predictions"] < VT + D["e2t"].shape[1]).all())
            collapsed = torch.nonzero(D["e2t"] >= 0)                                    # a collapsed slot is never drawn
            for b, c in collapsed.tolist():
                assert not bool((got["predictions"][b] == VT + c).any())
            again = _sample(net, seed, tau, top_k)
            assert all(torch.equal(again[k], got[k]) for k in got)                      # the same bits
            outs[fuse] = got
        assert torch.equal(outs[True]["predictions"], outs[False]["predictions"]) and torch.equal(outs[True]["lengths"], outs[False]["lengths"])
    finally:
        net.fuse_generator_argmax = net.fuse_generator_topk = True


@pytest.mark.parametrize("kind,tag", R.CASES)
def test_another_seed_differs_and_two_samples_are_the_first_two_of_four(nets, kind, tag):
    net = nets[kind, tag][0].network
    seed = R.SEEDS["%s_%s" % (kind, tag)][0]
    a, b = _sample(net, seed, 1.0, 0), _sample(net, seed + 1000, 1.0, 0)
    assert not torch.equal(a["predictions"], b["predictions"])
    two, four = _sample(net, seed, 1.0, 0, N=2), a
    assert torch.equal(two["predictions"], four["predictions"][:, :2]) and torch.equal(two["lengths"], four["lengths"][:, :2])
    assert torch.allclose(two["scores"], four["scores"][:, :2], rtol=1e-5, atol=1e-5)    # (the partials of another row count merge in another order)


@pytest.mark.parametrize("kind,tag", [("lstm", t) for t in AR.CASES] + [("gru", t) for t in GR.ACG_CASES])
def test_top_k_one_equals_the_greedy_decode_up_to_the_first_eos(kind, tag):
    net, c, g = AR.case(tag) if kind == "lstm" else GR.case("acg", tag)          # the unmodified greedy fixture
    max_len = int(AR.golden()["max_len"])
    net = _wrap(kind, tag, net, max_len).network
    greedy = net.decode(SRC.to(DEV), LENS.to(DEV), max_len, D["src_dict"], D["tgt_dict"], **MAPS)["predictions"].cpu()
    assert torch.equal(greedy, T(g["predictions"]))
    for seed, tau in ((0, 1.0), (12345, 0.25), ((1 << 64) - 1, 4.0)):
        got = _sample(net, seed, tau, 1, max_len=max_len, N=2)
        pred, ln = got["predictions"].cpu(), got["lengths"].cpu()
        for b in range(SRC.shape[0]):
            for n in range(2):
                L = int(ln[b, n])
                assert pred[b, n, :L].tolist() == greedy[b, :L].tolist()
                assert bool((pred[b, n, L:] == R.EOS).all())


@pytest.mark.parametrize("kind,tag", R.CASES)
def test_score_extended_reproduces_the_samples_scores_and_lengths(nets, kind, tag):
    r, sd, c, cell = nets[kind, tag]
    net = r.network
    seed = R.SCORE_SEEDS["%s_%s" % (kind, tag)]
    got = _sample(net, seed, 0.7, 0)
    pred = got["predictions"].cpu()
    live = torch.arange(R.MAXLEN).view(1, 1, -1) < got["lengths"].cpu().unsqueeze(2)
    assert not bool(((pred == 0) & live).any())                                          # a PAD-free seed (asserted on the CPU as well)
    cand = torch.cat((torch.full(pred.shape[:2] + (1,), R.BOS, dtype=torch.long), pred), 2)
    sc = net.score_extended(SRC.to(DEV), LENS.to(DEV), cand.to(DEV), src_dict=D["src_dict"], tgt_dict=D["tgt_dict"], **MAPS)
    assert torch.equal(sc["lengths"], got["lengths"])
    a = ("gru" if kind == "gru" else "lstm", sd, c, SRC, LENS, cand, D["idx"], D["e2t"], D["e2s"])
    lut = T(load_golden("acg_score")["tgt2src"])                                         # the table the dictionaries give
    ref, chain = SC.score(*a, tgt2src=lut), SC.score(*a, tgt2src=lut, dtype=torch.float32)
    n_split = SC.n_path(QL, R.MAXLEN) + 2
    ok, fig = SC.accept(sc, ref, chain, n_split)
    assert ok, fig
    ok, fig2 = SC.accept(dict(sc, scores=got["scores"]), ref, chain, n_split)            # the sampler's own sums against the scorer's reference
    print("acg sample round trip %s %s: scorer %.3g sampler %.3g" % (kind, tag, fig["scores"]["ratio"], fig2["scores"]["ratio"]))
    assert ok, fig2


def _collate(src, lens, tag):
    vocabs = AR.row_vocabs(src, lens)
    B = src.shape[0]
    toks = [[[AR.word(i) for i in src[b, :int(lens[b])].tolist()]] for b in range(B)]
    return dict(source_words=src.unsqueeze(1), source_lens=lens.unsqueeze(1), ids=["%s%d" % (tag, b) for b in range(B)], source_tokens=toks,
                target_tokens=[[["<s>", "a", "b", "</s>"]] for _ in range(B)], src_vocab=vocabs,
                src_map=[torch.tensor([vocabs[b][w] for w in toks[b][0]]) for b in range(B)])


def test_wrapper_returns_strings_with_copied_words_and_echoes_the_seed(nets):
    r = nets["lstm", "general"][0]
    ex = _collate(SRC, LENS, "q")
    B = SRC.shape[0]
    out = r.sample_extended(ex, R.N, seed=R.SEEDS["lstm_general"][0])
    assert out["seed"] == R.SEEDS["lstm_general"][0] and out["ex_ids"] == ex["ids"] and out["targets"] == [["a b"]] * B
    copied = 0
    for b in range(B):
        assert len(out["predictions"][b]) == R.N and all(isinstance(s, str) for s in out["predictions"][b])
        for n in range(R.N):
            want = []
            for wd in out["prediction_ids"][b, n].tolist():                              # tens2sen with the rows' dictionaries
                if wd == R.BOS:
                    continue
                if wd == R.EOS:
                    break
                want.append(D["tgt_dict"][wd] if wd < VT else ex["src_vocab"][b][wd - VT])
                copied += wd >= VT
            want = want or ["0"]
            att = out["attentions"][b, n].cpu()
            want = [ex["source_tokens"][b][0][int(att[i].argmax())] if w == "<unk>" else w for i, w in enumerate(want)]
            assert out["predictions"][b][n] == " ".join(want)
    assert copied >= 1
    torch.manual_seed(7)
    drawn = r.sample_extended(ex, 2, temperature=0.7, top_k=3)                           # seed=None: 63 bits from torch's CPU generator
    assert 0 <= drawn["seed"] < 2 ** 63
    replay = r.sample_extended(ex, 2, temperature=0.7, top_k=3, seed=drawn["seed"])
    assert torch.equal(replay["prediction_ids"], drawn["prediction_ids"]) and replay["predictions"] == drawn["predictions"]
    with pytest.raises(NotImplementedError, match="DESIGN.md section 28"):
        r.predict_samples(ex, 2)
    with pytest.raises(NotImplementedError, match="collapsed extended distribution"):
        r.network.decode_sample(SRC.to(DEV), LENS.to(DEV), R.MAXLEN, 2)
