"""GPU (-m gpu): ACG / ACGGRU.score_extended and CopyRecommender.score_extended (csrc/score.hip: the PAD-substituting generator form,
acg_score_finish_kernel; one nir_tf_attend in front) against the float64 restatement of tests/acg_score_ref.py and against the fixture computed
with the reference's own modules (tests/golden/acg_score.npz): all five ACG fixtures and one ACGGRU, N = 4 candidates with an early EOS, PAD
tails and tokens behind an EOS; B = 1; TL = 2; both generator forms; the nir_tf_attend front and the glue front; the recorded loss; the beam's
and the greedy decode's own tokens scored again."""
import pytest
import torch

import acg_beam_ref as BR
import acg_ref as AR
import acg_score_ref as R
import gru_dec_ref as GR
from conftest import T, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = BR.batch()
G = load_golden("acg_score")
SRC, LENS, CAND, LUT = D["src"], D["lens"], T(G["candidate_seq"]), T(G["tgt2src"])
QL, VT = SRC.shape[1], len(D["tgt_dict"])
MAPS = dict(src_map_idx=D["idx"], ext2tgt=D["e2t"], ext2src=D["e2s"])
CASES = [("lstm", t) for t in AR.CASES] + [("gru", "general")]


def _wrap(kind, tag, net, max_len=6):
    from context_attentive_ir_amd.wrappers import CopyRecommender
    args = GR.case_args("acg", tag, max_query_len=max_len) if kind == "gru" else AR.case_args(tag, max_query_len=max_len)
    r = CopyRecommender(args, D["src_dict"], D["tgt_dict"], net.state_dict())
    r.cuda()
    r.network.eval()
    return r


@pytest.fixture(scope="module")
def cases():
    """every case once: (wrapper on the GPU, state dict, cfg, fp64 scores, fp32 chain)"""
    out = {}
    for kind, tag in CASES:
        net, c, _ = AR.case(tag) if kind == "lstm" else GR.case("acg", tag)
        sd = net.state_dict()
        a = (kind, sd, c, SRC, LENS, CAND, D["idx"], D["e2t"], D["e2s"])
        out[kind, tag] = (_wrap(kind, tag, net), sd, c, R.score(*a, tgt2src=LUT), R.score(*a, tgt2src=LUT, dtype=torch.float32))
    return out


def _score(net, src=SRC, lens=LENS, cand=CAND, maps=MAPS, **kw):
    return net.score_extended(src.to(DEV), lens.to(DEV), cand.to(DEV), src_dict=D["src_dict"], tgt_dict=D["tgt_dict"], **maps, **kw)


def _n_split(net, T_):
    return R.n_path(QL, T_) + (2 if net._decoder_weights().keep.get("gen_frag") is not None else 0)


@pytest.fixture(scope="module")
def worst():
    w = {"tokens": 0.0, "scores": 0.0}
    yield w
    print("acg score models: largest ratios %s" % {k: round(v, 3) for k, v in w.items()})


@pytest.mark.parametrize("kind,tag", CASES)
def test_score_extended_matches_the_fp64_restatement_in_every_form(cases, worst, kind, tag):
    r, sd, c, ref, chain = cases[kind, tag]
    net = r.network
    B, N, TL = CAND.shape
    rec = T(G["logp_" + tag]) if kind == "lstm" else None
    counted = ref["token_logprobs"] != 0
    assert len({int(v) for v in ref["lengths"].reshape(-1)}) >= 3 and int(ref["lengths"].min()) == 1      # an early EOS, PAD tails
    outs = {}
    try:
        for fuse, front in ((True, True), (False, True), (True, False)):
            net.fuse_generator_argmax, net.fuse_teacher_front = fuse, front
            assert (net._decoder_weights().keep.get("gen_frag") is not None) == fuse                     # the form that was asked for ran
            got = _score(net)
            assert got["token_logprobs"].shape == (B, N, TL - 1) and got["scores"].shape == (B, N) and got["lengths"].dtype == torch.int64
            ok, fig = R.accept(got, ref, chain, _n_split(net, TL - 1))
            print("acg score %s %s fused=%s attend=%s: tokens ratio %.3g scores ratio %.3g" % (kind, tag, fuse, front, fig["token_logprobs"]["ratio"],
                                                                                         fig["scores"]["ratio"]))
            worst["tokens"] = max(worst["tokens"], fig["token_logprobs"]["ratio"])
            worst["scores"] = max(worst["scores"], fig["scores"]["ratio"])
            assert ok, fig
            lp = got["token_logprobs"].cpu()
            assert bool((lp[~counted] == 0).all())                                                       # PAD and behind the first EOS
            if rec is not None:                                                                          # the reference's own modules, float64
                assert float((lp.double() - rec)[counted].abs().max()) <= fig["token_logprobs"]["bound"] * ref["s"] + 1e-6
            again = _score(net)
            assert all(torch.equal(again[k], got[k]) for k in got)                                       # the same bits
            outs[fuse, front] = lp
        assert not torch.equal(outs[True, True], outs[False, True])                                      # two generator forms ran
    finally:
        net.fuse_generator_argmax = net.fuse_teacher_front = True
    net.check_ids()


def test_one_source_row_and_two_tokens(cases):
    r, sd, c, _, _ = cases["lstm", "general"]
    for b, tl in ((slice(0, 1), CAND.shape[2]), (slice(None), 2), (slice(1, 2), 2)):
        src, lens, cand = SRC[b], LENS[b], CAND[b, :, :tl].contiguous()
        maps = {k: v[b] for k, v in MAPS.items()}
        a = ("lstm", sd, c, src, lens, cand, maps["src_map_idx"], maps["ext2tgt"], maps["ext2src"])
        ref, chain = R.score(*a, tgt2src=LUT), R.score(*a, tgt2src=LUT, dtype=torch.float32)
        got = _score(r.network, src, lens, cand, maps)
        ok, fig = R.accept(got, ref, chain, _n_split(r.network, tl - 1))
        assert ok, (b, tl, fig)


def test_the_range_errors_of_decode_beam(cases):
    net = cases["lstm", "general"][0].network
    one = {k: (v[:, :1] if k != "src_map_idx" else v.clamp(max=0)) for k, v in MAPS.items()}
    with pytest.raises(ValueError, match="outside the copy generator's range"):
        _score(net, maps=one)
    with pytest.raises(ValueError, match="do not fit"):
        _score(net, maps=dict(MAPS, ext2src=D["e2s"][:, :-1]))
    out = _score(net, cand=torch.cat((CAND[:, :, :-1], torch.full_like(CAND[:, :, :1], VT + D["e2t"].shape[1])), 2))
    assert bool((out["token_logprobs"][:, 0, -1] == 0).all())                                             # past the end: reads 0 ...
    with pytest.raises(IndexError):
        net.check_ids()                                                                                  # ... and is flagged


@pytest.mark.parametrize("kind,tag", [("lstm", t) for t in AR.CASES])
def test_the_wrapper_gives_the_references_loss(cases, kind, tag):
    r = cases[kind, tag][0]
    vocabs = D["vocabs"]
    ex = dict(source_words=SRC.unsqueeze(1), source_lens=LENS.unsqueeze(1), target_words=D["tw"].unsqueeze(1), target_seq=D["ts"].unsqueeze(1),
              target_lens=D["tlen"].unsqueeze(1), src_map=D["maps"], alignment=D["als"], src_vocab=vocabs)
    out = r.score_extended(ex)
    want = float(G["loss_" + tag])
    assert abs(float(out["nll"]) - want) <= 1e-5 * abs(want), (float(out["nll"]), want)
    assert out["token_logprobs"].shape == (SRC.shape[0], 1, D["ts"].shape[1] - 1)
    n = int((D["ts"][:, 1:] != AR.PAD).sum())
    assert abs(float(out["perplexity"]) - float(torch.exp(torch.tensor(want * SRC.shape[0] / n)))) <= 1e-4 * float(out["perplexity"])
    ranked = r.score_extended(ex, candidates=CAND)
    assert ranked["ranking"].shape == CAND.shape[:2] and "nll" not in ranked
    assert torch.equal(ranked["ranking"], torch.sort(ranked["scores"], dim=-1, descending=True, stable=True)[1])
    own = dict(ex, candidate_seq=CAND.flip(1), candidate_rep=torch.ones_like(CAND))                        # the batch's own candidates and inputs ...
    again = r.score_extended(own, candidates=CAND)                                                         # ... are not mixed with explicit ones
    assert torch.equal(again["scores"], ranked["scores"])
    assert not torch.equal(r.score_extended(own)["scores"], ranked["scores"])


def test_the_beams_own_tokens_reproduce_its_scores_and_lengths():
    kind, tag, W = "lstm", "general", 3
    net, c, cell = BR.case(kind, tag, W)
    sd, L = net.state_dict(), BR.max_len(W)
    bargs = (sd, c, cell, SRC, LENS, L, W, D["idx"], D["e2t"], D["e2s"])
    bref = BR.decode(*bargs)
    bchain = BR.decode(*bargs, dtype=torch.float32, force=(bref["backptr"], bref["tokens"]))
    gnet = _wrap(kind, tag, net, L).network
    beam = gnet.decode_beam(SRC.to(DEV), LENS.to(DEV), L, W, D["src_dict"], D["tgt_dict"], **MAPS)
    cand = torch.cat((torch.full_like(beam["predictions"][..., :1], AR.BOS), beam["predictions"]), 2)
    got = _score(gnet, cand=cand)
    assert torch.equal(got["lengths"], beam["lengths"])
    w = gnet._decoder_weights().struct
    ok_b, fb = BR.accept_decode(beam, bref, bchain, L * (int(bool(w.rnn_whh_frag)) + int(bool(w.gen_frag) and gnet.fuse_generator_topk)))
    a = (kind, sd, c, SRC, LENS, cand.cpu(), D["idx"], D["e2t"], D["e2s"])
    ref, chain = R.score(*a, tgt2src=LUT), R.score(*a, tgt2src=LUT, dtype=torch.float32)
    ok_s, fs = R.accept(got, ref, chain, _n_split(gnet, L))
    assert ok_b and ok_s, (fb, fs)
    bound = fb["scores"]["bound"] * fb["scores"]["s"] + fs["scores"]["bound"] * fs["scores"]["s"]     # the sum of the two criteria's bounds
    diff = float((got["scores"] - beam["scores"]).abs().max())
    print("acg score of the beam's tokens: |score - beam| %.3g, bound %.3g" % (diff, bound))
    assert diff <= bound
    assert float((ref["scores"] - bref["scores"]).abs().max()) <= 1e-9                                   # the two restatements agree in float64


def test_the_greedy_decodes_own_tokens():
    kind, tag = "lstm", "general"
    net, c, g = AR.case(tag)
    sd, L = net.state_dict(), int(AR.golden()["max_len"])
    gnet = _wrap(kind, tag, net, L).network
    greedy = gnet.decode(SRC.to(DEV), LENS.to(DEV), L, D["src_dict"], D["tgt_dict"], **MAPS)
    assert torch.equal(greedy["predictions"].cpu(), T(g["predictions"]))
    cand = torch.cat((torch.full_like(greedy["predictions"][:, :1], AR.BOS), greedy["predictions"]), 1).unsqueeze(1)
    got = _score(gnet, cand=cand)
    beam = gnet.decode_beam(SRC.to(DEV), LENS.to(DEV), L, 1, D["src_dict"], D["tgt_dict"], **MAPS)
    assert torch.equal(beam["predictions"][:, 0], greedy["predictions"]) and torch.equal(got["lengths"], beam["lengths"])
    bargs = (sd, c, "LSTM", SRC, LENS, L, 1, D["idx"], D["e2t"], D["e2s"])                               # the width-1 search restated: the greedy walk
    bref = BR.decode(*bargs)
    bchain = BR.decode(*bargs, dtype=torch.float32, force=(bref["backptr"], bref["tokens"]))
    w = gnet._decoder_weights().struct
    ok_b, fb = BR.accept_decode(beam, bref, bchain, L * (int(bool(w.rnn_whh_frag)) + int(bool(w.gen_frag) and gnet.fuse_generator_topk)))
    a = (kind, sd, c, SRC, LENS, cand.cpu(), D["idx"], D["e2t"], D["e2s"])
    ref, chain = R.score(*a, tgt2src=LUT), R.score(*a, tgt2src=LUT, dtype=torch.float32)
    ok_s, fs = R.accept(got, ref, chain, _n_split(gnet, L))
    assert ok_b and ok_s, (fb, fs)
    bound = fb["scores"]["bound"] * fb["scores"]["s"] + fs["scores"]["bound"] * fs["scores"]["s"]     # the sum of the two criteria's bounds
    diff = float((got["scores"] - beam["scores"]).abs().max())
    print("acg score of the greedy tokens: |score - width-1 beam| %.3g, bound %.3g" % (diff, bound))
    assert diff <= bound
    assert float((ref["scores"] - bref["scores"]).abs().max()) <= 1e-9                                   # the two restatements agree in float64
    assert bool((got["token_logprobs"] <= 0).all()) and float(got["scores"].max()) < 0
