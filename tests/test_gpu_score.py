"""GPU (-m gpu): teacher-forced candidate scoring at model level (Seq2seq / Seq2seqGRU / HredQS .score_candidates, Recommender.score,
SessionRecommender.score) on the existing fixtures: the reference's recorded losses with the gold targets as the one candidate; score_ref's
criterion on candidates of unequal lengths, on B = 1 and on TL = 2, in the fused and the plain generator form; the beam's own scores and
lengths reproduced from its predictions; the ranking; and the id check."""
import pytest
import torch

import beam_ref as BR
import gru_dec_ref as GR
import hredqs_beam_ref as HB
import hredqs_ref as HQ
import score_ref as R
import seq2seq_ref as S
from conftest import T, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = {"s2s": load_golden("seq2seq"), "gru": {k[4:]: v for k, v in load_golden("seq2seq_gru").items() if k.startswith("s2s_")},
     "hredqs": load_golden("hredqs")}
MODELS = [("s2s", t) for t in S.CASES] + [("gru", "general"), ("gru", "mlp"), ("hredqs", "h64"), ("hredqs", "h1024")]
N_CAND = 4


def _load(kind, tag):
    """(wrapper on the GPU, state dict, cfg, src, lens, gold target_seq, gold target_words, tgt2src)"""
    from context_attentive_ir_amd.wrappers import Recommender, SessionRecommender
    if kind == "hredqs":
        net, c, a = HQ.case(tag)
        r = SessionRecommender(HQ.case_args(tag), None, None, net.state_dict())
        data = (a["source_words"], a["source_lens"], a["target_seq"], a["target_words"])
    else:
        net, c, a = S.case(tag) if kind == "s2s" else GR.case("s2s", tag)
        r = Recommender(S.case_args(tag) if kind == "s2s" else GR.case_args("s2s", tag), None, None, net.state_dict())
        data = tuple(T(G[kind][k]) for k in ("source_words", "source_lens", "target_seq", "target_words"))
    r.cuda()
    r.network.eval()
    return (r, net.state_dict(), c) + data + (T(G[kind]["tgt2src"]),)


@pytest.fixture(scope="module")
def models():
    return {m: _load(*m) for m in MODELS}


class _plain(object):
    """`with _plain(net, on)`: the scorer's plain generator form (the model's own switch), restored on exit; checks which form will run"""

    def __init__(self, net, on):
        self.net, self.on = net, on
        self.attr = "fast_decode" if hasattr(net, "fast_decode") else "fuse_generator_argmax"

    def __enter__(self):
        setattr(self.net, self.attr, not self.on)
        assert bool(self.net._decoder_weights().struct.gen_frag) == (not self.on)          # the fused form runs iff the fragment is there
        return self

    def __exit__(self, *exc):
        setattr(self.net, self.attr, True)


def _n_split(kind, src, cand, fused):
    return R.n_path(kind, src.shape[-1], cand.shape[-1] - 1, src.shape[1] if kind == "hredqs" else 0) + (2 if fused else 0)


def _ex(kind, src, lens, tseq, twords):
    if kind == "hredqs":
        return dict(source_words=src, source_lens=lens, target_seq=tseq, target_words=twords)
    return dict(source_words=src.unsqueeze(1), source_lens=lens.unsqueeze(1), target_seq=tseq.unsqueeze(1), target_words=twords.unsqueeze(1))


# ---- the recorded loss --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", MODELS)
def test_the_gold_target_gives_the_recorded_loss(models, kind, tag):
    r, sd, c, src, lens, tseq, twords, lut = models[kind, tag]
    want = float(G[kind]["loss_" + tag])
    for plain in (False, True):
        with _plain(r.network, plain):
            out = r.score(_ex(kind, src, lens, tseq, twords))
        assert set(out) == {"token_logprobs", "scores", "lengths", "nll", "perplexity"}
        lead = tuple(tseq.shape[:-1]) + (1,)
        assert out["scores"].shape == lead and out["lengths"].shape == lead and out["lengths"].dtype == torch.int64
        assert out["token_logprobs"].shape == lead + (tseq.shape[-1] - 1,) and out["token_logprobs"].dtype == torch.float32
        nll = float(out["nll"])
        print("score %s %s plain=%s: nll %.7g recorded %.7g rel %.3g" % (kind, tag, plain, nll, want, abs(nll - want) / want))
        assert abs(nll - want) <= 1e-5 * abs(want)
        n = (tseq[..., 1:] != R.PAD).sum()
        assert int(out["lengths"].sum()) == int(n)
        assert abs(float(out["perplexity"]) - float(torch.exp(-out["scores"].double().sum() / n))) <= 1e-5 * float(out["perplexity"])


# ---- the criterion ------------------------------------------------------------------------------------------------------------------------------------
def _settings(kind, src, lens, tseq):
    cand = R.candidates(tseq, N_CAND)
    yield "N=4", src, lens, cand
    yield "B=1", src[:1], lens[:1], cand[:1]
    yield "TL=2", src, lens, cand[..., :2].contiguous()


@pytest.mark.parametrize("kind,tag", MODELS)
def test_candidates_meet_the_criterion_in_both_forms(models, kind, tag):
    r, sd, c, src, lens, tseq, twords, lut = models[kind, tag]
    net = r.network
    for name, s_, l_, cand in _settings(kind, src, lens, tseq):
        ref = R.score(kind, sd, c, s_, l_, cand, tgt2src=lut)
        chain = R.score(kind, sd, c, s_, l_, cand, tgt2src=lut, dtype=torch.float32)
        for plain in (False, True):
            with _plain(net, plain):
                got = net.score_candidates(s_.to(DEV), l_.to(DEV), cand.to(DEV), tgt2src=lut.to(DEV))
                again = net.score_candidates(s_.to(DEV), l_.to(DEV), cand.to(DEV), tgt2src=lut.to(DEV))
            for k in ("token_logprobs", "scores", "lengths"):
                assert got[k].shape == ref[k].shape, (k, got[k].shape)
                assert torch.equal(got[k], again[k]), k                        # the same bits
            ok, fig = R.accept(got, ref, chain, _n_split(kind, s_, cand, not plain))
            print("score bound %s %s %s plain=%s: tokens %s scores %s" % (kind, tag, name, plain, fig["tokens"], fig["scores"]))
            assert ok, (name, plain, fig)
            if name == "N=4":
                assert int(got["lengths"].min()) == 1 and int(got["lengths"].max()) == cand.shape[-1] - 1
    net.check_ids()                                                            # nothing above was outside the vocabulary


def test_candidate_rep_is_what_the_decoder_is_fed(models):
    r, sd, c, src, lens, tseq, twords, lut = models["s2s", "general"]
    cand = R.candidates(tseq, 2)
    rep = (cand * 7 + 3) % int(G["s2s"]["vocab"])
    ref = R.score("s2s", sd, c, src, lens, cand, rep=rep)
    chain = R.score("s2s", sd, c, src, lens, cand, rep=rep, dtype=torch.float32)
    got = r.network.score_candidates(src.to(DEV), lens.to(DEV), cand.to(DEV), candidate_rep=rep.to(DEV))
    ok, fig = R.accept(got, ref, chain, _n_split("s2s", src, cand, True))
    assert ok, fig
    other = r.network.score_candidates(src.to(DEV), lens.to(DEV), cand.to(DEV), tgt2src=lut.to(DEV))
    assert not torch.equal(other["scores"], got["scores"])


# ---- the beam's own scores ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", [("s2s", "general"), ("gru", "mlp"), ("hredqs", "h64")])
def test_scoring_a_beams_predictions_reproduces_its_scores(kind, tag):
    W = 3
    if kind == "hredqs":
        assert (tag, W) in HB.case_w()
        cs, sd, ml = HB.load_case(tag), HB.perturbed(tag, W), HB.fixture_max_len(tag, W)
        src, lens, lut, c = cs["src"], cs["lens"], cs["lut"], None
        from context_attentive_ir_amd.wrappers import SessionRecommender
        r = SessionRecommender(HQ.case_args(tag), None, None, {k: v for k, v in sd.items()})
        bref = HB.decode(cs, sd, W, max_len=ml)
        bchain = HB.decode(cs, sd, W, torch.float32, force=(bref["backptr"], bref["tokens"]), max_len=ml)
        nsb, bmargin = HB.n_split(cs["QL"], cs["S"], True, ml), HB.MARGIN
    else:
        net0, c, cell, lut = BR.case(kind, tag, W)
        sd = net0.state_dict()
        src, lens, ml = BR.inputs()
        from context_attentive_ir_amd.wrappers import Recommender
        r = Recommender(S.case_args(tag) if kind == "s2s" else GR.case_args("s2s", tag), None, None, sd)
        bref = BR.decode(sd, c, cell, src, lens, ml, W, lut)
        bchain = BR.decode(sd, c, cell, src, lens, ml, W, lut, torch.float32, force=(bref["backptr"], bref["tokens"]))
        nsb, bmargin = 2 * ml, BR.MARGIN
    r.cuda()
    net = r.network.eval()
    beam = net.decode_beam(src.to(DEV), lens.to(DEV), ml, W, tgt2src=lut.to(DEV))
    pred = beam["predictions"]
    assert torch.equal(pred.cpu().reshape(bref["predictions"].shape), bref["predictions"])           # the fixture's condition: the float64 choices
    cand = torch.cat([torch.full_like(pred[..., :1], R.BOS), pred], -1)
    got = net.score_candidates(src.to(DEV), lens.to(DEV), cand, tgt2src=lut.to(DEV))
    assert torch.equal(got["lengths"], beam["lengths"])
    # the sum of the two criteria's bounds, each in absolute terms
    _, fb = BR.S.accept(beam["scores"].reshape(bref["scores"].shape), bref["scores"], bchain["scores"], nsb, bmargin)
    sref = R.score(kind, sd, c, src, lens, cand.cpu(), tgt2src=lut)
    schain = R.score(kind, sd, c, src, lens, cand.cpu(), tgt2src=lut, dtype=torch.float32)
    ok, fs = R.accept(got, sref, schain, _n_split(kind, src, cand, True))
    assert ok, fs
    tol = fb["bound"] * fb["s"] + fs["scores"]["bound"] * fs["scores"]["s"]
    diff = float((got["scores"] - beam["scores"]).abs().max())
    print("score vs beam %s %s: largest difference %.3g, tolerance %.3g" % (kind, tag, diff, tol))
    assert diff <= tol
    live = beam["lengths"] < ml                                                 # behind the first EOS nothing counts
    lp = got["token_logprobs"]
    pos = torch.arange(ml, device=DEV).expand_as(lp)
    assert bool((lp[pos >= beam["lengths"].unsqueeze(-1)] == 0).all()) and bool(live.any())


# ---- the ranking and the id check ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", [("s2s", "general"), ("hredqs", "h64")])
def test_ranking_is_the_stable_descending_argsort(models, kind, tag):
    r, sd, c, src, lens, tseq, twords, lut = models[kind, tag]
    cand = R.candidates(tseq, 6)
    cand[..., 5, :] = cand[..., 4, :]                                           # an exact tie: the smaller n first
    ex = _ex(kind, src, lens, tseq, twords)
    for norm in (False, True):
        out = r.score(ex, cand, length_normalize=norm)
        assert set(out) == {"token_logprobs", "scores", "lengths", "ranking"} and out["ranking"].shape == out["scores"].shape
        sc, ln = out["scores"].cpu(), out["lengths"].cpu()
        key = sc / ln.float() if norm else sc
        assert torch.equal(out["ranking"].cpu(), torch.sort(key, dim=-1, descending=True, stable=True)[1])
        rk = out["ranking"].cpu().reshape(-1, 6).tolist()
        assert all(row.index(4) < row.index(5) for row in rk)
    by_key = r.score(dict(ex, candidate_seq=cand))
    assert torch.equal(by_key["scores"], r.score(ex, cand)["scores"]) and "ranking" in by_key


def test_an_id_outside_the_target_vocabulary_surfaces_through_the_id_check(models):
    r, sd, c, src, lens, tseq, twords, lut = models["s2s", "general"]
    ex = _ex("s2s", src, lens, tseq, twords)
    cand = R.candidates(tseq, 3)
    cand[1, 2, 3] = int(G["s2s"]["tgt_vocab"]) + 5
    r.id_check, r.id_check_interval = "blocking", 1
    try:
        with pytest.raises(IndexError):
            r.score(ex, cand)
        bad_src = dict(ex, source_words=ex["source_words"].clone())
        bad_src["source_words"][0, 0, 0] = int(G["s2s"]["vocab"]) + 5
        with pytest.raises(IndexError):                                         # the way a bad source id does
            r.score(bad_src, R.candidates(tseq, 3))
        out = r.score(ex, R.candidates(tseq, 3))                                # the flag is clear again
        assert bool(torch.isfinite(out["scores"]).all())
    finally:
        r.id_check, r.id_check_interval = "deferred", 1
