"""GPU (-m gpu): teacher-forced candidate scoring under the session models (CARS / M_MATCH_TENSOR / MNSRF .score_candidates,
Multitask.score_suggestions) against the float64 restatement of tests/session_score_ref.py on session_beam_ref's five fixtures: candidates of
unequal lengths, B = 1 with S = 2, TL = 2, both generator forms and both attention forms (the form taken is read from the kernel names); the
beam's own scores and lengths reproduced from its predictions; the wrapper's nll against the model's own train-mode suggestion loss; the
ranking; and the id check.

Which case reaches which form: CARS (HD 512, P 256, VT 200, QL 6) runs the fused generator by default and the fused attention from 128 rows a
decode row on (the N = 26 setting; N = 4 runs the plain attention either way), MNSRF (H 1024) the fused generator; M_MATCH_TENSOR (H 300, no multiple of 32) has no generator fragments and runs the plain generator form either way."""
import contextlib
import ctypes as C
import re

import pytest
import torch

import session_beam_ref as SB
import session_score_ref as SS
from conftest import T, load_golden
from context_attentive_ir_amd import lib
from helpers import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODEL = {"cars": "CARS", "mmt": "M_MATCH_TENSOR", "mnsrf": "MNSRF"}
N_CAND = 4


def _model(kind, tag, sd=None):
    cs = SS.load_case(kind, tag)
    m = build_model(MODEL[kind], tgt_vocab_size=SS.vocab_tgt(cs), device=DEV, **cs.get("cfg", {}))
    if sd is not None:
        with torch.no_grad():
            for k in (SB.PRED2, "generator.bias"):
                if k in sd:
                    dict(m.named_parameters())[k].copy_(sd[k].to(DEV))
    return m


@pytest.fixture(scope="module")
def models():
    return {c: _model(*c) for c in SS.CASES}


def _kw(cs):
    kw = dict(states=(cs["dec_h"].unsqueeze(0).to(DEV), cs["dec_c"].unsqueeze(0).to(DEV)), src_dict=None, tgt_dict=None, batch_size=cs["B"],
              session_len=cs["SD"], tgt2src=cs["lut"].to(DEV) if cs.get("lut") is not None else None)
    if cs["kind"] == "cars":
        kw.update(encoded_source=cs["enc"].to(DEV), source_len=cs["lens"].to(DEV), session_attns=tuple(a.to(DEV) if a is not None else None for a in cs["attns"]))
    return kw


def _score(m, cs, cand, **extra):
    """cand [Bd, N, TL] on the CPU -> score_candidates' dict ([B, S-1, N, ..])"""
    Bd, N, TL = cand.shape
    out = m.score_candidates(candidate_seq=cand.view(cs["B"], cs["SD"], N, TL).to(DEV), **dict(_kw(cs), **extra))
    assert out["token_logprobs"].shape == (cs["B"], cs["SD"], N, TL - 1) and out["token_logprobs"].dtype == torch.float32
    assert out["scores"].shape == (cs["B"], cs["SD"], N) and out["lengths"].shape == (cs["B"], cs["SD"], N) and out["lengths"].dtype == torch.int64
    return out


def _profiled(fn):
    L = lib.load()
    buf = C.create_string_buffer(1 << 16)
    L.nir_profile_report(buf, len(buf))                     # drop what earlier tests left
    L.nir_profile_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.nir_profile_enable(0)
    L.nir_profile_report(buf, len(buf))
    return out, {re.sub(r"\[M=[^\]]*\]$", "", ln.rsplit(",", 2)[0]) for ln in buf.value.decode().strip().splitlines()}


@contextlib.contextmanager
def _switches(m, fuse_attention, fuse_generator):
    m.fuse_teacher_attention, m.fuse_generator_topk = fuse_attention, fuse_generator
    try:
        yield
    finally:
        m.fuse_teacher_attention, m.fuse_generator_topk = True, True


def _has_frag(m, cs):
    w = m.token_prob_predictor2.weight if cs["kind"] == "cars" else m.generator.weight
    return lib.load().nir_seq2seq_gen_frag_bytes(w.shape[0], w.shape[1]) > 0


def _sub_b1(cs):
    """B = 1, S = 2: the first decode row with its two source rows"""
    out = dict(cs, B=1, SD=1, dec_h=cs["dec_h"][:1], dec_c=cs["dec_c"][:1])
    if cs["kind"] == "cars":
        S = cs["SD"] + 1
        out.update(enc=cs["enc"][:2], lens=cs["lens"][:2], attns=[a[:1, :2] if a is not None else None for a in cs["attns"]],
                   session_cat=cs["session_cat"].view(cs["B"], S, -1)[:1, :2].reshape(2, -1) if cs["session_cat"] is not None else None)
    return out


def _settings(cs):
    cand = SS.candidates(cs, N_CAND)
    yield "N=4", cs, cand
    yield "B=1 S=2", _sub_b1(cs), cand[:1]
    yield "TL=2", cs, cand[..., :2].contiguous()
    if cs["kind"] == "cars":                                                    # N (TL - 1) >= 128 rows a decode row: the fused attention's range
        n = -(-SS.TF_MIN_G // (cand.shape[-1] - 1))
        yield "N=%d" % n, cs, SS.candidates(cs, n, seed=1)


# ---- the criterion ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", SS.CASES)
def test_candidates_meet_the_criterion_in_every_form(models, kind, tag):
    m = models[kind, tag]
    cs0 = SS.load_case(kind, tag)
    combos = [(a, g) for a in ((True, False) if kind == "cars" else (True,)) for g in (True, False)]
    for name, cs, cand in _settings(cs0):
        ref = SS.score(cs, cs["sd"], cand)
        chain = SS.score(cs, cs["sd"], cand, dtype=torch.float32)
        for fa, fg in combos:
            with _switches(m, fa, fg):
                got, names = _profiled(lambda: _score(m, cs, cand))
                again = _score(m, cs, cand)
            fused_gen = fg and _has_frag(m, cs)
            assert ("score_gen_target_kernel" in names) == fused_gen and ("score_row_kernel" in names) == (not fused_gen), names
            if kind == "cars":
                fa = fa and cand.shape[1] * (cand.shape[2] - 1) >= SS.TF_MIN_G   # the entry's own rule: plain below 128 rows a decode row
                assert ("tf_attend_fused_kernel" in names) == fa and ("tf_attend_plain_kernel" in names) == (not fa), names
            else:
                assert not any(n.startswith("tf_attend") for n in names), names
            for k in ("token_logprobs", "scores", "lengths"):
                assert torch.equal(got[k], again[k]), k                        # the same bits
            ok, fig = SS.accept(got, ref, chain, SS.n_split(kind, cand.shape[-1] - 1, fa, fused_gen))
            print("session score bound %s %s attn=%s gen=%s: tokens %s scores %s" % (SB.name(kind, tag), name, fa, fused_gen, fig["tokens"], fig["scores"]))
            assert ok, (name, fa, fg, fig)
        if name == "N=4":
            assert int(ref["lengths"].min()) == 1 and int(ref["lengths"].max()) == cand.shape[-1] - 1
    m.check_ids()                                                              # nothing above was outside the vocabulary


def test_candidate_rep_is_what_the_decoder_is_fed(models):
    cs, m = SS.load_case("cars", "full"), models["cars", "full"]
    cand = SS.candidates(cs, 2)
    rep = (cand * 7 + 3) % cs["V"]
    ref = SS.score(cs, cs["sd"], cand, rep=rep)
    chain = SS.score(cs, cs["sd"], cand, rep=rep, dtype=torch.float32)
    got = _score(m, cs, cand, candidate_rep=rep.view(cs["B"], cs["SD"], 2, -1).to(DEV))
    ok, fig = SS.accept(got, ref, chain, SS.n_split("cars", cand.shape[-1] - 1, False, True))      # 10 rows a decode row: the plain attention
    assert ok, fig
    assert not torch.equal(_score(m, cs, cand)["scores"], got["scores"])


# ---- the beam's own scores ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", SB.WIDE_CASES)
def test_scoring_a_beams_predictions_reproduces_its_scores(kind, tag):
    W = 3
    cs, sd = SS.load_case(kind, tag), SB.perturbed(kind, tag, W)
    m = _model(kind, tag, sd)
    bref = SB.decode(cs, sd, W)
    bchain = SB.decode(cs, sd, W, torch.float32, force=(bref["backptr"], bref["tokens"]))
    beam = m.decode_beam(max_len=cs["max_len"], beam_size=W, **_kw(cs))
    pred = beam["predictions"]                                                  # [B, S-1, W, max_len]
    assert torch.equal(pred.cpu().reshape(bref["predictions"].shape), bref["predictions"])           # the fixture's condition: the float64 choices
    cand = torch.cat([torch.full_like(pred[..., :1], SS.BOS), pred], -1)
    got = m.score_candidates(candidate_seq=cand, **_kw(cs))
    assert torch.equal(got["lengths"], beam["lengths"])
    ok_b, fb = SB.accept_decode(beam, bref, bchain, SB.n_split(True, True, cs["max_len"]))
    assert ok_b, fb
    c3 = cand.cpu().reshape(cs["B"] * cs["SD"], W, -1)
    sref = SS.score(cs, sd, c3)
    schain = SS.score(cs, sd, c3, dtype=torch.float32)
    ok, fs = SS.accept(got, sref, schain, SS.n_split(kind, cs["max_len"], W * cs["max_len"] >= SS.TF_MIN_G, True))
    assert ok, fs
    tol = fb["scores"]["bound"] * fb["scores"]["s"] + SS.score_bound_abs(fs)     # the sum of the two criteria's bounds, each in absolute terms
    diff = float((got["scores"] - beam["scores"]).abs().max())
    print("session score vs beam %s: largest difference %.3g, tolerance %.3g" % (SB.name(kind, tag), diff, tol))
    assert diff <= tol
    lp = got["token_logprobs"]
    pos = torch.arange(cs["max_len"], device=DEV).expand_as(lp)
    assert bool((lp[pos >= beam["lengths"].unsqueeze(-1)] == 0).all())          # behind the first EOS nothing counts


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------------------------------
def _wrapper(model, fixture):
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import Multitask
    from helpers import SEED
    g = load_golden(fixture)
    V = int(g["meta_vocab"])
    args = default_args(model, src_vocab_size=V, tgt_vocab_size=V if model == "CARS" else 50, dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0,
                        regularize_coeff=0.0)
    w = Multitask(args)
    fill_module_(w.network, SEED)
    w.cuda()
    keys = ("source_words", "source_lens", "document_words", "document_lens", "document_labels", "target_words", "target_seq", "target_lens")
    return w, {k: T(g["b0_" + k]) for k in keys}


@pytest.mark.parametrize("model,fixture", [("CARS", "cars_train"), ("MNSRF", "mnsrf_train"), ("M_MATCH_TENSOR", "m_match_tensor_train")])
def test_nll_is_the_models_own_train_mode_suggestion_loss(model, fixture):
    w, ex = _wrapper(model, fixture)
    out = w.score_suggestions(ex)
    assert set(out) == {"click_scores", "token_logprobs", "scores", "lengths", "nll", "perplexity"}
    B, S = ex["source_words"].shape[:2]
    assert out["scores"].shape == (B, S - 1, 1) and out["lengths"].shape == (B, S - 1, 1)
    assert torch.equal(out["click_scores"], w.predict(ex, suggest=False)["click_scores"])          # exactly predict()'s
    w.network.train()
    with torch.no_grad():
        loss = w.network(source_rep=ex["source_words"].to(DEV), source_len=ex["source_lens"].to(DEV), target_rep=ex["target_words"].to(DEV),
                         target_len=ex["target_lens"].to(DEV), target_seq=ex["target_seq"].to(DEV), document_rep=ex["document_words"].to(DEV),
                         document_len=ex["document_lens"].to(DEV), document_label=ex["document_labels"].to(DEV))["suggestion_loss"]
    w.network.eval()
    nll, want = float(out["nll"]), float(loss)
    print("score_suggestions %s: nll %.7g train-mode suggestion loss %.7g rel %.3g" % (model, nll, want, abs(nll - want) / abs(want)))
    assert abs(nll - want) <= 1e-5 * abs(want)
    n = (ex["target_seq"][..., 1:] != SS.PAD).sum()
    assert int(out["lengths"].sum()) == int(n)
    assert abs(float(out["perplexity"]) - float(torch.exp(-out["scores"].double().sum() / n))) <= 1e-5 * float(out["perplexity"])


@pytest.mark.parametrize("kind,tag", SS.CASES)
def test_ranking_is_the_float64_ranking(models, kind, tag):
    """on candidates whose float64 gaps are ten times the bound (tests/test_session_score_host.py asserts that on the CPU)"""
    cs, m = SS.load_case(kind, tag), models[kind, tag]
    cand = SS.ranking_candidates(cs)
    ref = SS.score(cs, cs["sd"], cand)
    got = _score(m, cs, cand)
    shape = ref["scores"].shape
    for norm in (False, True):
        key = got["scores"] / got["lengths"].clamp(min=1) if norm else got["scores"]
        rk = torch.sort(key, dim=-1, descending=True, stable=True)[1].cpu().reshape(shape)
        want = torch.sort(ref["scores"] / ref["lengths"].double() if norm else ref["scores"], dim=-1, descending=True, stable=True)[1]
        assert torch.equal(rk, want), norm


def test_the_wrappers_ranking_and_the_id_check():
    w, ex = _wrapper("CARS", "cars_train")
    B, S = ex["source_words"].shape[:2]
    V = int(load_golden("cars_train")["meta_vocab"])
    cand = SS.R.candidates(ex["target_seq"], 6, V)
    cand[..., 5, :] = cand[..., 4, :]                                           # an exact tie: the smaller n first
    for norm in (False, True):
        out = w.score_suggestions(ex, cand, length_normalize=norm)
        assert set(out) == {"click_scores", "token_logprobs", "scores", "lengths", "ranking"} and out["ranking"].shape == (B, S - 1, 6)
        sc, ln = out["scores"].cpu(), out["lengths"].cpu()
        key = sc / ln.float() if norm else sc
        assert torch.equal(out["ranking"].cpu(), torch.sort(key, dim=-1, descending=True, stable=True)[1])
        assert all(row.index(4) < row.index(5) for row in out["ranking"].cpu().reshape(-1, 6).tolist())
    by_key = w.score_suggestions(dict(ex, candidate_seq=cand))
    assert torch.equal(by_key["scores"], w.score_suggestions(ex, cand)["scores"]) and "ranking" in by_key
    from context_attentive_ir_amd.eval import MRR
    assert 0.0 < MRR(by_key["ranking"].cpu().reshape(-1, 6), torch.nn.functional.one_hot(torch.zeros(B * (S - 1), dtype=torch.long), 6)) <= 1.0
    bad = cand.clone()
    bad[1, 0, 2, 3] = V + 5
    w.id_check, w.id_check_interval = "blocking", 1
    try:
        with pytest.raises(IndexError):
            w.score_suggestions(ex, bad)
        out = w.score_suggestions(ex, cand)                                     # the flag is clear again
        assert bool(torch.isfinite(out["scores"]).all())
    finally:
        w.id_check, w.id_check_interval = "deferred", 1


def test_cars_without_the_recommender_returns_the_scoring_keys_as_none():
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.wrappers import Multitask
    g = load_golden("cars_train")
    V = int(g["meta_vocab"])
    w = Multitask(default_args("CARS", src_vocab_size=V, tgt_vocab_size=V, turn_recommender_off=True))
    w.cuda()
    ex = {k: T(g["b0_" + k]) for k in ("source_words", "source_lens", "document_words", "document_lens", "document_labels", "target_words", "target_seq")}
    out = w.score_suggestions(ex)
    assert out["click_scores"] is not None and all(out[k] is None for k in ("token_logprobs", "scores", "lengths", "nll", "perplexity"))
    out = w.score_suggestions(ex, ex["target_seq"].unsqueeze(2))
    assert out["click_scores"] is not None and all(out[k] is None for k in ("token_logprobs", "scores", "lengths", "ranking"))
