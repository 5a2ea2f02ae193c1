"""GPU (-m gpu): the sampling decode of Seq2seq and Seq2seqGRU (csrc/sample.hip, Seq2seq.decode_sample, Recommender.predict_samples) against the
float64 restatement of tests/sample_ref.py on the beam fixtures (the greedy fixtures with a noisy generator bias), N = 4 samples per row, at
tau 1 and 0.7, over the whole vocabulary and over the top 3: tokens and lengths exactly (tests/test_sample_host.py keeps every step's gap
above 10 x the token bound for these seeds), scores, token log-probabilities and attentions inside their bounds; the generator and step forms
against the same reference; top_k = 1 against the greedy decode; score_candidates on the samples of all seven fixtures, and on samples that hold PAD; repeatability, another seed, and the (source
row, sample) keying of the noise."""
import pytest
import torch

import beam_ref
import gru_dec_ref as GR
import sample_ref as R
import score_ref
import seq2seq_ref as S
from conftest import T, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = load_golden("seq2seq")
SRC, LENS, MAXLEN = beam_ref.inputs()
QL, VT = SRC.shape[1], int(G["tgt_vocab"])
SPECIAL = ["<blank>", "<unk>", "<s>", "</s>"]
TGT_DICT = [SPECIAL[i] if i < 4 else "w%d" % i for i in range(VT)]
SRC_DICT = {TGT_DICT[i]: int(s) for i, s in enumerate(G["tgt2src"])}        # src_dict[tgt_dict[i]] = tgt2src[i]
N = R.N
CASE_SET = [(k, t, tau, top_k) for k, t in R.CASES for tau, top_k in R.SETTINGS]


def _wrap(kind, tag, net):
    from context_attentive_ir_amd.wrappers import Recommender
    args = S.case_args(tag) if kind == "s2s" else GR.case_args("s2s", tag)
    r = Recommender(args, SRC_DICT, TGT_DICT, net.state_dict())
    r.cuda()
    r.network.eval()
    return r


class _Cases(object):
    """every fixture once on the GPU; the float64 decode and the float32 chain forced along it per setting, on demand"""
    def __init__(self):
        self.nets, self.refs = {}, {}

    def net(self, kind, tag):
        if (kind, tag) not in self.nets:
            net, c, cell, lut = R.case(kind, tag)
            self.nets[kind, tag] = (_wrap(kind, tag, net), net.state_dict(), c, cell, lut)
        return self.nets[kind, tag]

    def ref(self, kind, tag, tau, top_k, seed=None):
        seed = R.SEEDS["%s_%s" % (kind, tag)] if seed is None else seed
        key = (kind, tag, tau, top_k, seed)
        if key not in self.refs:
            _, sd, c, cell, lut = self.net(kind, tag)
            ref = R.decode(sd, c, cell, SRC, LENS, MAXLEN, N, seed, tau, top_k, lut)
            chain = R.decode(sd, c, cell, SRC, LENS, MAXLEN, N, seed, tau, top_k, lut, dtype=torch.float32, force=ref["tokens"])
            self.refs[key] = (ref, chain)
        return self.refs[key]


@pytest.fixture(scope="module")
def cases():
    return _Cases()


def _decode(net, tau, top_k, seed, src=SRC, lens=LENS, n=N):
    return net.decode_sample(src.to(DEV), lens.to(DEV), MAXLEN, n, temperature=tau, top_k=top_k, seed=seed, src_dict=SRC_DICT, tgt_dict=TGT_DICT)


def _n_split(net, top_k):
    """split products on the path of a score: one recurrent (fp16-term step) and one generator product (fused form) per step"""
    w = net._decoder_weights().struct
    fused = bool(w.gen_frag) and (net.fuse_generator_topk if top_k else net.fuse_generator_argmax)
    return MAXLEN * (int(bool(w.rnn_whh_frag)) + int(fused))


@pytest.mark.parametrize("kind,tag,tau,top_k", CASE_SET)
def test_decode_sample_matches_the_fp64_restatement(cases, kind, tag, tau, top_k):
    r = cases.net(kind, tag)[0]
    ref, chain = cases.ref(kind, tag, tau, top_k)
    net, seed = r.network, R.SEEDS["%s_%s" % (kind, tag)]
    got = _decode(net, tau, top_k, seed)
    B = SRC.shape[0]
    assert got["predictions"].shape == (B, N, MAXLEN) and got["predictions"].dtype == torch.int64
    assert got["token_logprobs"].shape == (B, N, MAXLEN) and got["token_logprobs"].dtype == torch.float32
    assert got["scores"].shape == (B, N) and got["lengths"].shape == (B, N) and got["lengths"].dtype == torch.int64
    assert got["attentions"].shape == (B, N, MAXLEN, QL)
    w = net._decoder_weights().struct
    assert w.gen_frag and w.rnn_whh_frag and w.rnn_gate_fold                 # the fast forms ran
    ok, fig = R.accept_decode(got, ref, chain, _n_split(net, top_k))
    print("sample bound %s %s tau=%g top_k=%d: scores %s token_logprobs %s attentions %s" % (kind, tag, tau, top_k, fig["scores"], fig["token_logprobs"],
                                                                                           fig["attentions"]))
    assert ok, fig
    pred, tlp = got["predictions"].cpu(), got["token_logprobs"].cpu()
    behind = (torch.cumsum((pred == R.EOS).long(), 2) - (pred == R.EOS).long()) > 0
    assert bool((pred[behind] == R.EOS).all()) and bool((tlp[behind] == 0).all())        # frozen: EOS at log-probability 0
    masked = (torch.arange(QL).view(1, 1, 1, QL) >= LENS.view(-1, 1, 1, 1)).expand(-1, N, MAXLEN, -1)
    assert bool((got["attentions"].cpu()[masked] == 0).all())
    again = _decode(net, tau, top_k, seed)
    for k in ("predictions", "token_logprobs", "scores", "lengths", "attentions"):
        assert torch.equal(again[k], got[k]), k                              # the same seed: the same bits
    other = _decode(net, tau, top_k, seed + R.OTHER_SEED)
    assert not torch.equal(other["predictions"], got["predictions"])         # (asserted on the restatement by tests/test_sample_host.py)


@pytest.mark.parametrize("kind,tag", [("s2s", "dot"), ("s2s", "wide"), ("gru", "general")])
def test_generator_and_step_forms_draw_the_same_tokens(cases, kind, tag):
    r = cases.net(kind, tag)[0]
    net, seed = r.network, R.SEEDS["%s_%s" % (kind, tag)]
    try:
        for tau, top_k in ((0.7, 0), (1.0, 3)):
            ref, chain = cases.ref(kind, tag, tau, top_k)
            for fold, fuse in ((True, False), (False, True), (False, False)):
                net.fold_decoder_step, net.fuse_generator_argmax, net.fuse_generator_topk = fold, fuse, fuse
                w = net._decoder_weights().struct
                assert bool(w.rnn_whh_frag) == fold
                got = _decode(net, tau, top_k, seed)
                ok, fig = R.accept_decode(got, ref, chain, _n_split(net, top_k))
                print("sample bound %s %s tau=%g top_k=%d fold=%s fuse=%s: scores %s" % (kind, tag, tau, top_k, fold, fuse, fig["scores"]))
                assert ok, fig
    finally:
        net.fold_decoder_step = net.fuse_generator_argmax = net.fuse_generator_topk = True


def test_beyond_the_row_cap_the_plain_form_runs(cases):
    """fuse_sample_max_rows (default suggest.FUSE_SAMPLE_MAX_ROWS): above it the whole-vocabulary form takes the plain generator -- the bits of
    fuse_generator_argmax = False -- and the top-k form is untouched"""
    from context_attentive_ir_amd.multitask import suggest
    assert suggest.FUSE_SAMPLE_MAX_ROWS == 512
    net = cases.net("s2s", "general")[0].network
    fused, fused_k = _decode(net, 0.7, 0, 9), _decode(net, 0.7, 3, 9)
    try:
        net.fuse_sample_max_rows = SRC.shape[0] * N - 1
        capped, capped_k = _decode(net, 0.7, 0, 9), _decode(net, 0.7, 3, 9)
        net.fuse_sample_max_rows = SRC.shape[0] * N
        at_cap = _decode(net, 0.7, 0, 9)
    finally:
        del net.fuse_sample_max_rows
    try:
        net.fuse_generator_argmax = False
        plain = _decode(net, 0.7, 0, 9)
    finally:
        net.fuse_generator_argmax = True
    for k in ("predictions", "token_logprobs", "scores", "attentions"):
        assert torch.equal(capped[k], plain[k]) and torch.equal(at_cap[k], fused[k]) and torch.equal(capped_k[k], fused_k[k]), k
    assert not torch.equal(fused["token_logprobs"], plain["token_logprobs"])  # two different kernels ran


@pytest.mark.parametrize("kind,tag", R.CASES)
def test_top_k_one_is_the_greedy_decode_up_to_the_first_eos(cases, kind, tag):
    net = cases.net(kind, tag)[0].network
    greedy = net.decode(SRC.to(DEV), LENS.to(DEV), MAXLEN, SRC_DICT, TGT_DICT)["predictions"].cpu()
    for seed in (3, 4):
        got = _decode(net, 0.3, 1, seed)
        pred, ln = got["predictions"].cpu(), got["lengths"].cpu()
        for b in range(SRC.shape[0]):
            for n in range(N):
                upto = int(ln[b, n])
                assert torch.equal(pred[b, n, :upto], greedy[b, :upto]), (b, n)
                assert bool((pred[b, n, upto:] == R.EOS).all())


def _round_trip(cases, kind, tag, seed):
    """(the sample, score_candidates on [BOS] + its predictions, the sum of the two criteria's bounds on a score)"""
    r, sd, c, cell, lut = cases.net(kind, tag)
    net = r.network
    tau, top_k = 0.7, 0
    ref, chain = cases.ref(kind, tag, tau, top_k, seed)
    got = _decode(net, tau, top_k, seed)
    assert torch.equal(got["predictions"].cpu(), ref["predictions"])
    cand = torch.cat((torch.full((SRC.shape[0], N, 1), R.BOS, dtype=torch.int64), got["predictions"].cpu()), 2)
    sc = net.score_candidates(SRC.to(DEV), LENS.to(DEV), cand.to(DEV), src_dict=SRC_DICT, tgt_dict=TGT_DICT)
    _, fig = R.accept_decode(got, ref, chain, _n_split(net, top_k))
    k = "gru" if kind == "gru" else "s2s"
    sref = score_ref.score(k, sd, c, SRC, LENS, cand, tgt2src=lut)
    schain = score_ref.score(k, sd, c, SRC, LENS, cand, tgt2src=lut, dtype=torch.float32)
    ok, sfig = score_ref.accept(sc, sref, schain, score_ref.n_path(k, QL, MAXLEN) + 2)
    assert ok, sfig
    return got, sc, fig["scores"]["bound"] * fig["scores"]["s"] + sfig["scores"]["bound"] * sfig["scores"]["s"]


@pytest.mark.parametrize("kind,tag", R.CASES)
def test_score_candidates_reproduces_the_samples_scores(cases, kind, tag):
    """all seven fixtures, each with a seed whose samples hold no PAD (sample_ref.SCORE_SEEDS; gaps and PAD asserted on the CPU)"""
    got, sc, bound = _round_trip(cases, kind, tag, R.SCORE_SEEDS["%s_%s" % (kind, tag)])
    assert bool((got["predictions"] != score_ref.PAD).all())
    assert torch.equal(sc["lengths"], got["lengths"])
    diff = float((sc["scores"].cpu() - got["scores"].cpu()).abs().max())
    print("score_candidates on the samples %s %s: |difference| %.3g, bound %.3g" % (kind, tag, diff, bound))
    assert diff <= bound


def test_score_candidates_leaves_out_a_sampled_pad(cases):
    """the caveat of the contract: a whole-vocabulary draw can emit PAD; score_candidates does not count that position, so it returns the score
    less the PAD positions' token_logprobs in front of the first EOS, and the length less their number"""
    kind, tag, seed = R.PAD_CASE
    got, sc, bound = _round_trip(cases, kind, tag, seed)
    pred, tlp, ln = got["predictions"].cpu(), got["token_logprobs"].cpu(), got["lengths"].cpu()
    pad = (pred == score_ref.PAD) & (torch.arange(MAXLEN).view(1, 1, -1) < ln.unsqueeze(2))
    assert bool(pad.any())
    assert torch.equal(sc["lengths"].cpu(), ln - pad.sum(2))
    want = got["scores"].cpu().double() - (tlp.double() * pad).sum(2)
    diff = float((sc["scores"].cpu().double() - want).abs().max())
    print("score_candidates on samples with PAD %s %s: |difference| %.3g, bound %.3g" % (kind, tag, diff, bound))
    assert diff <= bound
    assert float((sc["scores"].cpu() - got["scores"].cpu()).abs().max()) > bound    # (and the uncorrected scores do differ)


def test_a_source_rows_samples_do_not_depend_on_the_batch(cases):
    net = cases.net("s2s", "general")[0].network
    keep, more = R.appended_batch(LENS)
    a = _decode(net, 1.0, 0, 5, SRC[keep], LENS[keep])
    b = _decode(net, 1.0, 0, 5, SRC[more], LENS[more])
    nk = keep.numel()
    assert torch.equal(b["predictions"][:nk], a["predictions"]) and torch.equal(b["lengths"][:nk], a["lengths"])
    _, sd, c, cell, lut = cases.net("s2s", "general")
    want = R.decode(sd, c, cell, SRC[more], LENS[more], MAXLEN, N, 5, 1.0, 0, lut)
    assert float(want["gaps"].min()) > 1e-4                                   # (no near-tie in this draw)
    assert torch.equal(b["predictions"].cpu(), want["predictions"])


def test_more_samples_extend_the_draw(cases):
    """sample n of a source row is the same draw whatever N is: the counter holds n, not the row"""
    net = cases.net("gru", "mlp")[0].network
    a, b = _decode(net, 1.0, 0, 8, n=2), _decode(net, 1.0, 0, 8, n=5)
    assert torch.equal(b["predictions"][:, :2], a["predictions"]) and b["predictions"].shape[1] == 5


def test_predict_samples_shapes_strings_and_seed(cases):
    r = cases.net("s2s", "general")[0]
    B = SRC.shape[0]
    toks = [[["<s>"] + ["s%d_%d" % (b, j) for j in range(int(LENS[b]))] + ["</s>"]] for b in range(B)]
    ex = dict(source_words=SRC.unsqueeze(1), source_lens=LENS.unsqueeze(1), ids=["q%d" % b for b in range(B)], source_tokens=toks,
              target_tokens=[[["<s>", "a", "b", "</s>"]] for _ in range(B)], src_vocab=None)
    seed = R.SEEDS["s2s_general"]
    ref = cases.ref("s2s", "general", 0.7, 3)[0]
    out = r.predict_samples(ex, N, temperature=0.7, top_k=3, seed=seed)
    assert out["seed"] == seed and out["prediction_ids"].shape == (B, N, MAXLEN) and out["attentions"].shape == (B, N, MAXLEN, QL)
    assert out["token_logprobs"].shape == (B, N, MAXLEN) and out["scores"].shape == (B, N) and out["lengths"].shape == (B, N)
    assert torch.equal(out["prediction_ids"].cpu(), ref["predictions"]) and torch.equal(out["lengths"].cpu(), ref["lengths"])
    assert out["ex_ids"] == ex["ids"] and out["targets"] == [["a b"]] * B
    for b in range(B):
        assert len(out["predictions"][b]) == N
        for n in range(N):
            want = []
            for wd in ref["predictions"][b, n].tolist():
                if wd == 2:
                    continue
                if wd == 3:
                    break
                want.append(TGT_DICT[wd])
            want = want or ["0"]
            att = out["attentions"][b, n].cpu()
            want = [toks[b][0][int(att[i].argmax())] if w == "<unk>" else w for i, w in enumerate(want)]
            assert out["predictions"][b][n] == " ".join(want)
    plain = dict(source_words=SRC.unsqueeze(1), source_lens=LENS.unsqueeze(1))
    torch.manual_seed(77)
    drawn = r.predict_samples(plain, 2)
    assert "predictions" not in drawn and 0 <= drawn["seed"] < 2 ** 63
    replay = r.predict_samples(plain, 2, seed=drawn["seed"])
    assert torch.equal(replay["prediction_ids"], drawn["prediction_ids"]) and torch.equal(replay["scores"], drawn["scores"])
    again = r.predict_samples(plain, 2)
    assert again["seed"] != drawn["seed"]                                     # the default generator moved on
    with pytest.raises(ValueError):
        r.predict_samples(plain, 0)
