"""GPU (-m gpu): the sampling decode of HredQS and the session models (csrc/session_sample.hip; CARS / M_MATCH_TENSOR / MNSRF / HredQS
.decode_sample; SessionRecommender.predict_session_samples, Multitask.predict_samples) against the float64 restatement of
tests/session_sample_ref.py on the golden weights as they are, at the seeds stored there (their gaps are asserted on the CPU by
tests/test_session_sample_host.py, so tokens and lengths are demanded exactly).

Which case reaches which form by default: the CARS goldens (HD 512, P 256) and MNSRF (H 1024) run the folded step and the fused generator,
M_MATCH_TENSOR (H 300, no multiple of 32) the fp32 step and the plain generator; HredQS h64 / h96 / h256 run sample_gen_kernel<BeamRowsSplit, 4>
and h1024 <BeamRowsSplit, 2> on the split state, `fast_decode = False` the entry's plain form."""
import contextlib

import pytest
import torch

import score_ref
import session_sample_ref as R
import session_score_ref as SS
from test_gpu_hredqs_beam import TGT_DICT, _form, _wrap
from test_gpu_session_beam import FAST, _model, _wrapper
from test_gpu_session_score import _kw, _profiled

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = R.N
OUT_KEYS = ("predictions", "token_logprobs", "scores", "lengths")


@pytest.fixture(scope="module")
def nets():
    """one network on the GPU per case, the golden weights as they are"""
    out = {}
    for key in R.KEYS:
        c = R.load(key)
        out[key] = _wrap(key[3:]).network if c["family"] == "hredqs" else _model(c["cs"]["kind"], c["cs"]["tag"])
    return out


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(key, tau, top_k, seed, n=N):
        k = (key, tau, top_k, seed, n)
        if k not in cache:
            ref = R.decode(key, seed, tau, top_k, n=n)
            cache[k] = (ref, R.decode(key, seed, tau, top_k, n=n, dtype=torch.float32, force=ref["tokens"]))
        return cache[k]
    return get


def _decode(net, key, tau, top_k, seed, n=N, cs=None):
    c = R.load(key)
    cs = c["cs"] if cs is None else cs
    if c["family"] == "hredqs":
        out = net.decode_sample(cs["src"].to(DEV), cs["lens"].to(DEV), c["max_len"], n, temperature=tau, top_k=top_k, seed=seed, tgt2src=cs["lut"].to(DEV))
        lead = (cs["B"], cs["S"])
    else:
        out = net.decode_sample(max_len=c["max_len"], num_samples=n, temperature=tau, top_k=top_k, seed=seed, **_kw(cs))
        lead = (cs["B"], cs["SD"])
    assert set(out) == set(OUT_KEYS)                                             # there are no attentions
    assert out["predictions"].shape == lead + (n, c["max_len"]) and out["predictions"].dtype == torch.int64
    assert out["token_logprobs"].shape == lead + (n, c["max_len"]) and out["token_logprobs"].dtype == torch.float32
    assert out["scores"].shape == lead + (n,) and out["lengths"].shape == lead + (n,) and out["lengths"].dtype == torch.int64
    return out


def _forms(key):
    """(folded step, fused generator) a case reaches by default"""
    c = R.load(key)
    return (True, True) if c["family"] == "hredqs" else FAST[c["cs"]["kind"]]


@contextlib.contextmanager
def _plain(net, key):
    """the entry's plain forms: HredQS `fast_decode = False`; the session models both generator switches and the step's fold"""
    if R.load(key)["family"] == "hredqs":
        with _form(net, "plain"):
            yield
        return
    had = "fold_decoder_step" in net.__dict__
    old = getattr(net, "fold_decoder_step", True)
    net.fold_decoder_step, net.fuse_generator_topk, net.fuse_generator_argmax = False, False, False
    try:
        yield
    finally:
        net.fuse_generator_topk = True
        del net.fuse_generator_argmax
        if had:
            net.fold_decoder_step = old
        else:
            del net.fold_decoder_step


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    print("session sample: largest ratios e / bound (scores, token_logprobs) per (case, form): %s"
          % {k: tuple(round(x, 3) for x in v) for k, v in w.items()})


def _accept(key, got, ref, chain, forms, worst, what):
    c = R.load(key)
    ok, fig = R.accept_decode(got, ref, chain, R.n_split(c, *forms))
    if fig.get("scores") != "non-finite":
        r = R.ratios(fig)
        old = worst.get((key, what), (0.0, 0.0))
        worst[key, what] = (max(old[0], r[0]), max(old[1], r[1]))
    print("session sample bound %s %s: %s" % (key, what, fig))
    assert ok, (key, what, fig)


@pytest.mark.parametrize("key", R.KEYS)
def test_decode_sample_matches_the_fp64_restatement_in_every_setting(nets, refs, worst, key):
    net = nets[key]
    for si, (tau, top_k) in enumerate(R.SETTINGS):
        seed = R.SEEDS[key][si]
        ref, chain = refs(key, tau, top_k, seed)
        got = _decode(net, key, tau, top_k, seed)
        _accept(key, got, ref, chain, _forms(key), worst, "default")
        again = _decode(net, key, tau, top_k, seed)
        for k in OUT_KEYS:
            assert torch.equal(again[k], got[k]), k                              # the same bits
        other = _decode(net, key, tau, top_k, seed + R.OTHER_SEED)
        assert not torch.equal(other["predictions"], got["predictions"])          # another seed: another draw


@pytest.mark.parametrize("key", R.KEYS)
def test_fused_and_plain_forms_draw_the_same_tokens(nets, refs, worst, key):
    net = nets[key]
    for si, (tau, top_k) in enumerate(R.SETTINGS):
        seed = R.SEEDS[key][si]
        ref, chain = refs(key, tau, top_k, seed)
        fused = _decode(net, key, tau, top_k, seed)
        with _plain(net, key):
            plain = _decode(net, key, tau, top_k, seed)
        _accept(key, plain, ref, chain, (False, False), worst, "plain")
        assert torch.equal(plain["predictions"], fused["predictions"]) and torch.equal(plain["lengths"], fused["lengths"])


@pytest.mark.parametrize("key", ["cars_full", "mnsrf"])
def test_beyond_the_row_cap_the_plain_generator_runs_and_draws_the_same_tokens(nets, key):
    net = nets[key]
    seed = R.SEEDS[key][0]
    fused, names = _profiled(lambda: _decode(net, key, 1.0, 0, seed))
    assert any(n.startswith("sample_gen_kernel") for n in names) and "sample_row_kernel" not in names, names
    net.fuse_sample_max_rows = R.load(key)["Bd"] * N - 1
    try:
        plain, names = _profiled(lambda: _decode(net, key, 1.0, 0, seed))
    finally:
        del net.fuse_sample_max_rows
    assert "sample_row_kernel" in names and not any(n.startswith("sample_gen_kernel") for n in names), names
    assert torch.equal(plain["predictions"], fused["predictions"]) and torch.equal(plain["lengths"], fused["lengths"])


def test_hredqs_fast_form_draws_on_the_split_state(nets):
    net = nets["hq_h64"]
    _, names = _profiled(lambda: _decode(net, "hq_h64", 1.0, 0, 1))
    assert any(n.startswith("hq_sample_gen_kernel") for n in names) and "sample_row_kernel" not in names, names
    _, names = _profiled(lambda: _decode(net, "hq_h64", 1.0, 3, 1))
    assert any(n.startswith("hq_beam_gen_topk_kernel") for n in names) and "sample_topk_select_kernel" in names, names
    net.fuse_sample_max_rows = 1                                                # a cap of HredQS's own: the entry's plain form beyond it
    try:
        _, names = _profiled(lambda: _decode(net, "hq_h64", 1.0, 0, 1))
    finally:
        del net.fuse_sample_max_rows
    assert "sample_row_kernel" in names and not any(n.startswith("hq_sample_gen_kernel") for n in names), names


@pytest.mark.parametrize("key", R.KEYS)
def test_top_k_one_is_the_recorded_greedy_decode_for_every_seed(nets, key):
    c = R.load(key)
    want = c["cs"]["greedy"].reshape(c["Bd"], -1)
    for seed in (1, 2, (1 << 63) + 7):
        got = _decode(nets[key], key, 0.3, 1, seed)
        pred, ln = got["predictions"].cpu().reshape(c["Bd"], N, -1), got["lengths"].cpu().reshape(c["Bd"], N)
        for i in range(c["Bd"]):
            for n in range(N):                                                  # up to each row's first EOS
                assert torch.equal(pred[i, n, :int(ln[i, n])], want[i, :int(ln[i, n])]), (key, seed, i, n)
                assert bool((pred[i, n, int(ln[i, n]):] == R.SR.EOS).all())


@pytest.mark.parametrize("key", R.KEYS)
def test_score_candidates_reproduces_the_samples_scores(nets, refs, worst, key):
    """every case at the seed whose samples hold no PAD in front of their first EOS (asserted on the CPU)"""
    c = R.load(key)
    cs, net = c["cs"], nets[key]
    tau, top_k = R.SCORE_SETTING
    seed = R.SCORE_SEEDS[key]
    ref, chain = refs(key, tau, top_k, seed)
    got = _decode(net, key, tau, top_k, seed)
    assert torch.equal(got["predictions"].cpu().reshape(ref["predictions"].shape), ref["predictions"])
    _, fig = R.accept_decode(got, ref, chain, R.n_split(c, *_forms(key)))
    pred = got["predictions"]
    cand = torch.cat([torch.full_like(pred[..., :1], R.SR.BOS), pred], -1)
    c3 = cand.cpu().reshape(c["Bd"], N, -1)
    if c["family"] == "hredqs":
        sc = net.score_candidates(cs["src"].to(DEV), cs["lens"].to(DEV), cand, tgt2src=cs["lut"].to(DEV))
        c4 = cand.cpu()
        sref = score_ref.score("hredqs", cs["sd"], cs["cfg"], cs["src"], cs["lens"], c4, tgt2src=cs["lut"])
        schain = score_ref.score("hredqs", cs["sd"], cs["cfg"], cs["src"], cs["lens"], c4, tgt2src=cs["lut"], dtype=torch.float32)
        ok, sfig = score_ref.accept(sc, sref, schain, score_ref.n_path("hredqs", cs["QL"], c["max_len"], cs["S"]) + 2)
        sbound = sfig["scores"]["bound"] * sfig["scores"]["s"]
    else:
        sc = net.score_candidates(candidate_seq=cand, **_kw(cs))
        sref, schain = SS.score(cs, cs["sd"], c3), SS.score(cs, cs["sd"], c3, dtype=torch.float32)
        ok, sfig = SS.accept(sc, sref, schain, SS.n_split(cs["kind"], c["max_len"], N * c["max_len"] >= SS.TF_MIN_G, _forms(key)[1]))
        sbound = SS.score_bound_abs(sfig)
    assert ok, sfig
    assert torch.equal(sc["lengths"], got["lengths"])
    bound = fig["scores"]["bound"] * fig["scores"]["s"] + sbound                # the sum of the two criteria's bounds, each in absolute terms
    diff = float((sc["scores"] - got["scores"]).abs().max())
    print("score_candidates on the samples %s: |difference| %.3g, bound %.3g" % (key, diff, bound))
    assert diff <= bound


@pytest.mark.parametrize("key", ["cars_full", "mnsrf"])
def test_a_decode_rows_samples_do_not_depend_on_the_batch_around_it(nets, key):
    """the first session alone against the whole batch: the noise is keyed by (decode row, sample), not by the sample row"""
    c = R.load(key)
    cs = c["cs"]
    SD = cs["SD"]
    one = dict(cs, B=1, dec_h=cs["dec_h"][:SD], dec_c=cs["dec_c"][:SD])
    if cs["kind"] == "cars":
        one.update(enc=cs["enc"][:SD + 1], lens=cs["lens"][:SD + 1], attns=[a[:1] if a is not None else None for a in cs["attns"]])
    for tau, top_k in ((1.0, 0), (0.7, 3)):
        whole = _decode(nets[key], key, tau, top_k, 5)
        alone = _decode(nets[key], key, tau, top_k, 5, cs=one)
        assert torch.equal(alone["predictions"][0], whole["predictions"][0]) and torch.equal(alone["lengths"][0], whole["lengths"][0])
        assert float((alone["scores"][0] - whole["scores"][0]).abs().max()) <= 1e-4 * float(whole["scores"].abs().max())
        assert not torch.equal(whole["predictions"][0], whole["predictions"][1])


@pytest.mark.parametrize("key", ["cars_full", "hq_h96", "hq_h1024"])
def test_more_samples_extend_the_draw(nets, key):
    for tau, top_k in ((1.0, 0), (0.7, 3)):
        four, two = _decode(nets[key], key, tau, top_k, 3, n=4), _decode(nets[key], key, tau, top_k, 3, n=2)
        for k in ("predictions", "lengths"):
            assert torch.equal(four[k][:, :, :2], two[k]), k
        assert float((four["scores"][:, :, :2] - two["scores"]).abs().max()) <= 1e-4 * float(four["scores"].abs().max())


# ---- the wrappers -------------------------------------------------------------------------------------------------------------------------------
def _strings(ids, words):
    out = []
    for row in ids.tolist():
        sent = []
        for wd in row:
            if wd == R.SR.BOS:
                continue
            if wd == R.SR.EOS:
                break
            sent.append(words[wd])
        out.append(" ".join(sent) if sent else "0")
    return out


def test_predict_session_samples_shapes_strings_and_the_returned_seed(refs):
    key = "hq_h64"
    c = R.load(key)
    cs = c["cs"]
    r = _wrap("h64")
    B, S, ml = cs["B"], cs["S"], c["max_len"]
    assert r.args.max_query_len == ml
    lens = cs["lens"]
    toks = [[["<s>"] + ["s%d_%d_%d" % (b, s, j) for j in range(int(lens[b, s]))] + ["</s>"] for s in range(S)] for b in range(B)]
    tgts = [[["<s>", "t%d_%d" % (b, s), "x", "</s>"] for s in range(S)] for b in range(B)]
    ex = dict(source_words=cs["src"], source_lens=lens, ids=["q%d_" % b for b in range(B)], source_tokens=toks, target_tokens=tgts, src_vocab=None,
              session_len=S, batch_size=B)
    seed = R.SEEDS[key][1]
    tau, top_k = R.SETTINGS[1]
    out, one = r.predict_session_samples(ex, N, temperature=tau, top_k=top_k, seed=seed), r.predict(ex)
    assert out["seed"] == seed and out["prediction_ids"].shape == (B, S, N, ml) and out["token_logprobs"].shape == (B, S, N, ml)
    assert out["scores"].shape == (B, S, N) and out["lengths"].shape == (B, S, N)
    ref, _ = refs(key, tau, top_k, seed)
    ids = out["prediction_ids"].cpu()
    assert torch.equal(ids.reshape(B * S, N, ml), ref["predictions"])           # through the dictionaries' table
    assert out["ex_ids"] == one["ex_ids"] and out["targets"] == one["targets"] and out["src_sequences"] == one["src_sequences"]
    assert len(out["predictions"]) == B * S
    for s in range(S):                                                          # step-major, like predict()
        for b in range(B):
            assert out["predictions"][s * B + b] == _strings(ids[b, s], TGT_DICT)
    bare = dict(source_words=cs["src"], source_lens=lens)
    a = r.predict_session_samples(bare, 2)                                       # seed=None: drawn on the host, returned
    assert set(a) == {"prediction_ids", "token_logprobs", "scores", "lengths", "seed"} and 0 <= a["seed"] < 2 ** 63
    b = r.predict_session_samples(bare, 2, seed=a["seed"])
    for k in ("prediction_ids", "token_logprobs", "scores", "lengths"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(r.predict_session_samples(bare, 2, seed=a["seed"] ^ 1)["prediction_ids"], a["prediction_ids"])
    assert r._graphs is None or r._graphs.captures == 0                         # eager: nothing is captured


@pytest.mark.parametrize("kind,tag", [("cars", "full"), ("mmt", ""), ("mnsrf", "")])
def test_multitask_predict_samples(refs, kind, tag):
    key = R.SB.name(kind, tag)
    c = R.load(key)
    cs = c["cs"]
    w, ex = _wrapper(kind, tag, None)
    B, S = ex["source_words"].shape[:2]
    ml = w.args.max_query_len
    greedy = w.predict(ex)
    a = w.predict_samples(ex, N)
    assert {"click_scores", "prediction_ids", "token_logprobs", "scores", "lengths", "seed"} <= set(a) and 0 <= a["seed"] < 2 ** 63
    assert a["prediction_ids"].shape == (B, S - 1, N, ml) and a["token_logprobs"].shape == (B, S - 1, N, ml)
    assert a["scores"].shape == (B, S - 1, N) and a["lengths"].shape == (B, S - 1, N)
    assert torch.equal(a["click_scores"].cpu(), greedy["click_scores"].cpu())    # exactly predict()'s: the same kernels
    b = w.predict_samples(ex, N, seed=a["seed"])
    for k in ("prediction_ids", "token_logprobs", "scores", "lengths"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(w.predict_samples(ex, N, seed=a["seed"] ^ 1)["prediction_ids"], a["prediction_ids"])
    assert w._graphs is None or w._graphs.captures <= 1                         # (predict() may have captured its own graph; sampling adds none)
    text = dict(ex, ids=["s%d" % i for i in range(B)], session_len=S, batch_size=B,
                source_tokens=[[["<s>", "q%d_%d" % (i, s), "</s>"] for s in range(S)] for i in range(B)],
                target_tokens=[[["<s>", "t%d_%d" % (i, s), "</s>"] for s in range(S - 1)] for i in range(B)])
    out, one = w.predict_samples(text, 3, temperature=0.7, top_k=3, seed=11), w.predict(text)
    assert out["ex_ids"] == one["ex_ids"] and out["targets"] == one["targets"] and out["src_sequences"] == one["src_sequences"]
    ids = out["prediction_ids"].cpu()
    assert len(out["predictions"]) == B * (S - 1)
    for sidx in range(S - 1):                                                   # step-major, like predict()
        for i in range(B):
            assert out["predictions"][sidx * B + i] == _strings(ids[i, sidx], w.tgt_dict)
    assert cs["max_len"] == ml


def test_cars_with_the_recommender_off_returns_none_keys():
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.wrappers import Multitask
    w, ex = _wrapper("cars", "full", None)
    off = Multitask(default_args("CARS", src_vocab_size=200, tgt_vocab_size=200, turn_recommender_off=True))
    off.cuda()
    o = off.predict_samples({k: v for k, v in ex.items() if torch.is_tensor(v)}, 4)
    assert o["click_scores"] is not None
    assert all(o[k] is None for k in ("prediction_ids", "token_logprobs", "scores", "lengths", "seed"))
