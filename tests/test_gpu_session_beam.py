"""GPU (-m gpu): the session models' beam search (csrc/beam.hip: nir_beam_cars_decode / nir_beam_plain_decode; CARS / M_MATCH_TENSOR /
MNSRF .decode_beam; Multitask.predict_beam) against the float64 restatement of tests/session_beam_ref.py on the beam fixtures; the generator
and step forms against each other; eager against graph replay; bitwise repeatability; W = 1 against the greedy decode on the unmodified
goldens; and the envelope of the two entries at the C ABI.

Which test reaches which form: the CARS goldens (HD 512, P 256, VT 200) and MNSRF (H 1024, VT 50) run the folded step AND the fused generator
by default; M_MATCH_TENSOR (H 300, no multiple of 32) runs the fp32 step and the GEMM + row top-k.  The envelope's plain decoder (H 32) runs
both fast forms and, with both switched off, both plain ones."""
import contextlib

import pytest
import torch

import beam_ref as BR
import session_beam_ref as R
from conftest import T, load_golden
from context_attentive_ir_amd import lib
from context_attentive_ir_amd.multitask import suggest
from helpers import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASE_W = [(k, t, W) for k, t in R.CASES for W in R.widths(k, t)]
MODEL = {"cars": "CARS", "mmt": "M_MATCH_TENSOR", "mnsrf": "MNSRF"}
FAST = {"cars": (True, True), "mnsrf": (True, True), "mmt": (False, False)}              # (folded step, fused generator) the goldens reach


def _model(kind, tag, sd=None):
    cs = R.load_case(kind, tag)
    m = build_model(MODEL[kind], tgt_vocab_size=cs["lut"].shape[0], device=DEV, **cs.get("cfg", {}))
    if sd is not None:
        with torch.no_grad():
            for k in (R.PRED2, "generator.bias"):
                if k in sd:
                    dict(m.named_parameters())[k].copy_(sd[k].to(DEV))
    return m


@pytest.fixture(scope="module")
def cases():
    """every (case, W) once: (case, model on the GPU with the fixture's noise, fp64 decode, fp32 decode forced along the fp64 choices)"""
    out = {}
    for kind, tag, W in CASE_W:
        cs, sd = R.load_case(kind, tag), R.perturbed(kind, tag, W)
        ref = R.decode(cs, sd, W)
        chain = R.decode(cs, sd, W, torch.float32, force=(ref["backptr"], ref["tokens"]))
        out[kind, tag, W] = (cs, _model(kind, tag, sd), ref, chain)
    return out


def _decode(m, cs, W, greedy=False):
    kw = dict(states=(cs["dec_h"].unsqueeze(0).to(DEV), cs["dec_c"].unsqueeze(0).to(DEV)), max_len=cs["max_len"], src_dict=None, tgt_dict=None,
              batch_size=cs["B"], session_len=cs["SD"], tgt2src=cs["lut"].to(DEV))
    if cs["kind"] == "cars":
        kw.update(encoded_source=cs["enc"].to(DEV), source_len=cs["lens"].to(DEV), session_attns=tuple(a.to(DEV) if a is not None else None for a in cs["attns"]))
    if greedy:
        return m.decode(use_cuda=True, **kw)
    out = m.decode_beam(beam_size=W, return_backptr=True, **kw)
    Bd = cs["B"] * cs["SD"]
    assert out["predictions"].shape == (cs["B"], cs["SD"], W, cs["max_len"]) and out["predictions"].dtype == torch.int64
    assert out["scores"].shape == (cs["B"], cs["SD"], W) and out["lengths"].shape == (cs["B"], cs["SD"], W) and out["backptr"].shape == (cs["max_len"], Bd, W)
    return out


def _forms(m, cs):
    """(folded step, fused generator) of the last decode, read from the model's packs"""
    fused = m.fuse_generator_topk and getattr(m, "_pgen_beam", None) is not None and m._pgen_beam.val is not None
    if cs["kind"] == "cars":
        return bool(m._decoder_weights().struct.rnn_whh_frag), fused
    return m._pdec_plain.val is not None, fused


def _same_bits(a, b):
    for k in ("predictions", "scores", "lengths", "backptr"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("kind,tag,W", CASE_W)
def test_beam_decode_matches_the_fp64_restatement(cases, kind, tag, W):
    cs, m, ref, chain = cases[kind, tag, W]
    got = _decode(m, cs, W)
    forms = _forms(m, cs)
    assert forms == FAST[kind], forms                                           # the forms the module docstring names ran
    ok, fig = R.accept_decode(got, ref, chain, R.n_split(*forms, cs["max_len"]))
    print("session beam bound %s W=%d forms=%s: %s" % (R.name(kind, tag), W, forms, fig))
    assert ok, fig
    sc = got["scores"].reshape(-1, W).cpu()
    assert bool((sc[:, :-1] >= sc[:, 1:]).all())                                # best beam first
    _same_bits(_decode(m, cs, W), got)                                          # the same bits


@contextlib.contextmanager
def _switches(m, fold, fuse):
    had = "fold_decoder_step" in m.__dict__
    old = getattr(m, "fold_decoder_step", True)
    m.fold_decoder_step, m.fuse_generator_topk = fold, fuse
    try:
        yield
    finally:
        m.fuse_generator_topk = True
        if had:
            m.fold_decoder_step = old
        else:
            del m.fold_decoder_step


@pytest.mark.parametrize("kind,tag", [("cars", "full"), ("cars", "qoff"), ("mnsrf", "")])
def test_generator_and_step_forms_agree_in_every_token(cases, kind, tag):
    cs, m, ref, chain = cases[kind, tag, 4]
    for fold, fuse in ((True, False), (False, True), (False, False)):
        with _switches(m, fold, fuse):
            got = _decode(m, cs, 4)
            assert _forms(m, cs) == (fold, fuse)
            ok, fig = R.accept_decode(got, ref, chain, R.n_split(fold, fuse, cs["max_len"]))
            print("session beam bound %s fold=%s fuse=%s: %s" % (R.name(kind, tag), fold, fuse, fig))
            assert ok, fig


@pytest.mark.parametrize("kind,tag", R.CASES)
def test_width_one_equals_the_greedy_decode_token_for_token(kind, tag):
    cs = R.load_case(kind, tag)
    m = _model(kind, tag)                                                       # the unmodified golden
    greedy = _decode(m, cs, 1, greedy=True)["predictions"]
    beam = _decode(m, cs, 1)
    assert torch.equal(greedy.reshape(cs["greedy"].shape).cpu(), cs["greedy"])
    assert torch.equal(beam["predictions"][:, :, 0], greedy)
    assert bool((beam["backptr"] == 0).all()) and bool((beam["lengths"] == cs["max_len"]).all())   # (the goldens never emit EOS)


# ---- the wrapper --------------------------------------------------------------------------------------------------------------------------------
def _wrapper(kind, tag, sd):
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.wrappers import Multitask
    cs = R.load_case(kind, tag)
    g = load_golden({"cars": "cars_decode", "mmt": "m_match_tensor", "mnsrf": "mnsrf"}[kind])
    args = default_args(MODEL[kind], src_vocab_size=cs["V"], tgt_vocab_size=cs["lut"].shape[0], max_query_len=cs["max_len"], **cs.get("cfg", {}))
    VT = cs["lut"].shape[0]
    tgt_dict = ["t%d" % i for i in range(VT)]
    src_dict = _Dict({tgt_dict[i]: int(s) for i, s in enumerate(cs["lut"])}, cs["V"])
    w = Multitask(args, src_dict, tgt_dict, {k: v for k, v in _model(kind, tag, sd).state_dict().items()})
    w.cuda()
    ex = {k: T(g[k]) for k in ("source_words", "source_lens", "document_words", "document_lens")}
    if kind == "cars":
        ex["document_labels"] = T(g["document_labels"])
    return w, ex


class _Dict(dict):
    """src_dict[word] -> id with the vocabulary's length (the wrapper reads len(src_dict) as the vocabulary size)"""

    def __init__(self, d, n):
        super().__init__(d)
        self._n = n

    def __len__(self):
        return self._n


def _roll(ex):
    return {k: v.roll(1, 0).contiguous() for k, v in ex.items()}


@pytest.mark.parametrize("kind,tag", [("cars", "full"), ("mmt", ""), ("mnsrf", "")])
def test_predict_beam_eager_graph_replay_and_click_scores(kind, tag):
    w, ex = _wrapper(kind, tag, R.perturbed(kind, tag, 4))
    ex2 = _roll(ex)                                                             # the same shape, other contents
    w.args.predict_graphs = False
    eager = [w.predict_beam(e, 4) for e in (ex, ex2)]
    greedy = [w.predict(e) for e in (ex, ex2)]
    assert w._graphs is None or w._graphs.captures == 0
    w.args.predict_graphs = True
    w.predict_graph_min_calls = 2
    w.clear_predict_graphs()
    outs = [w.predict_beam(ex, 4) for _ in range(3)] + [w.predict_beam(ex2, 4)]  # eager, captured and replayed, replayed, replayed on other contents
    assert w._graphs is not None and w._graphs.captures == 1 and w._graphs.replays >= 3
    B, S = ex["source_words"].shape[:2]
    for o, want, gr in zip(outs, [eager[0]] * 3 + [eager[1]], [greedy[0]] * 3 + [greedy[1]]):
        assert {"click_scores", "prediction_ids", "scores", "lengths"} <= set(o)
        assert o["prediction_ids"].shape == (B, S - 1, 4, w.args.max_query_len)
        for k in ("prediction_ids", "scores", "lengths"):
            assert torch.equal(o[k].cpu(), want[k].cpu()), k
        assert torch.equal(o["click_scores"].cpu(), gr["click_scores"].cpu())    # exactly predict()'s: the same kernels
    assert not torch.equal(eager[0]["scores"], eager[1]["scores"])             # (the two batches do differ)


def test_predict_beam_text_and_the_recommender_switch():
    w, ex = _wrapper("cars", "full", R.perturbed("cars", "full", 4))
    B, S = ex["source_words"].shape[:2]
    ex = dict(ex, ids=["s%d" % b for b in range(B)], session_len=S, batch_size=B,
              source_tokens=[[["<s>", "q%d_%d" % (b, s), "</s>"] for s in range(S)] for b in range(B)],
              target_tokens=[[["<s>", "t%d_%d" % (b, s), "</s>"] for s in range(S - 1)] for b in range(B)])
    out, one = w.predict_beam(ex, 4), w.predict(ex)
    assert out["ex_ids"] == one["ex_ids"] and out["targets"] == one["targets"] and out["src_sequences"] == one["src_sequences"]
    ids = out["prediction_ids"].cpu()
    assert len(out["predictions"]) == B * (S - 1)
    for sidx in range(S - 1):                                                   # step-major, like predict()
        for b in range(B):
            row = out["predictions"][sidx * B + b]
            assert len(row) == 4
            for k in range(4):
                sent = []
                for wd in ids[b, sidx, k].tolist():
                    if wd == BR.BOS:
                        continue
                    if wd == BR.EOS:
                        break
                    sent.append(w.tgt_dict[wd])
                assert row[k] == (" ".join(sent) if sent else "0")
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.wrappers import Multitask
    off = Multitask(default_args("CARS", src_vocab_size=200, tgt_vocab_size=200, turn_recommender_off=True))
    off.cuda()
    o = off.predict_beam({k: v for k, v in ex.items() if torch.is_tensor(v)}, 4)
    assert o["prediction_ids"] is None and o["click_scores"] is not None


# ---- the envelope at the C ABI --------------------------------------------------------------------------------------------------------------------
H_ENV, E_ENV, V_ENV = 32, 8, 40


def _plain_problem(Bd, seed):
    """a decoder without attention at the smallest dims that reach both fast forms (H 32), detinit weights; the generator is scaled up so that
    the candidates lie apart"""
    from context_attentive_ir_amd.detinit import det_tensor
    d = lambda n, shape, scale=None: det_tensor("session_beam.env." + n, shape, seed, scale)       # noqa: E731
    sd = {R.TABLE: d("table", (V_ENV, E_ENV), 0.5), "decoder.decoder.rnn.weight_ih_l0": d("wih", (4 * H_ENV, E_ENV)),
          "decoder.decoder.rnn.weight_hh_l0": d("whh", (4 * H_ENV, H_ENV)), "decoder.decoder.rnn.bias_ih_l0": d("bih", (4 * H_ENV,)),
          "decoder.decoder.rnn.bias_hh_l0": d("bhh", (4 * H_ENV,)), "generator.weight": d("gw", (V_ENV, H_ENV), 2.0), "generator.bias": d("gb", (V_ENV,), 1.0)}
    sd["generator.bias"][BR.EOS] += 1.0
    lut = (torch.arange(V_ENV) * 7 + 3) % (V_ENV + 2)                           # two targets map outside the source vocabulary: fed back as <unk>
    return dict(kind="plain", sd=sd, dec_h=d("h0", (Bd, H_ENV), 1.0), dec_c=d("c0", (Bd, H_ENV), 1.0), lut=lut, V=V_ENV, B=Bd, SD=1)


def _plain_call(cs, W, max_len, fast, rows=None):
    """rows: the Bd handed to the entry when it is not the buffers' (0: an empty batch over live buffers)"""
    L = lib.load()
    sd = {k: v.to(DEV).contiguous() for k, v in cs["sd"].items()}
    p = [sd["decoder.decoder.rnn." + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    t, gw, gb = sd[R.TABLE], sd["generator.weight"], sd["generator.bias"]
    Bd = cs["dec_h"].shape[0]
    fold = gfrag = None
    if fast:
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        wfrag = torch.empty(L.nir_lstm_step_whh_frag_bytes(H_ENV), dtype=torch.uint8, device=DEV)
        lib.check(L.nir_lstm_step_pack_whh_frag(lib.ptr(p[1]), H_ENV, lib.ptr(wfrag), lib.ptr(flag), lib.stream()), "pack whh")
        gfrag = torch.empty(L.nir_seq2seq_gen_frag_bytes(V_ENV, H_ENV), dtype=torch.uint8, device=DEV)
        lib.check(L.nir_seq2seq_pack_gen_frag(lib.ptr(gw), V_ENV, H_ENV, lib.ptr(gfrag), lib.ptr(flag), lib.stream()), "pack gen")
        assert int(flag.item()) == 0
        fold = (lib.fold_lstm_table(t, p[0], p[2], p[3], H_ENV, 1, "f32"), wfrag)
    out = suggest.beam_outputs(Bd, W, max_len, DEV, True)
    for v in out.values():
        v.fill_(-7)
    h, c, lut = cs["dec_h"].to(DEV), cs["dec_c"].to(DEV), cs["lut"].to(DEV)
    nb = L.nir_beam_plain_decode_workspace_bytes(Bd, H_ENV, V_ENV, W, max_len, int(fast), int(fast))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    rc = L.nir_beam_plain_decode(lib.ptr(h), lib.ptr(c), Bd if rows is None else rows, H_ENV, lib.ptr(t), V_ENV, E_ENV, lib.ptr(p[0]), lib.ptr(p[1]), lib.ptr(p[2]), lib.ptr(p[3]),
                                 lib.ptr(gw), lib.ptr(gb), V_ENV, lib.ptr(lut), BR.BOS, max_len, lib.ptr(fold[0]) if fold else None,
                                 lib.ptr(fold[1]) if fold else None, lib.ptr(gfrag), W, lib.ptr(ws), nb, lib.ptr(out["predictions"]), lib.ptr(out["scores"]),
                                 lib.ptr(out["lengths"]), lib.ptr(out["backptr"]), lib.stream())
    torch.cuda.synchronize()
    return rc, out


def _gapped(make, W, max_len, limit=60):
    """the first seed whose float64 decode keeps every gap >= 1e-3 and whose free float32 decode agrees -- decided on the CPU"""
    for seed in range(1, limit):
        cs = dict(make(seed), max_len=max_len)
        ref = R.decode(cs, cs["sd"], W)
        free = R.decode(cs, cs["sd"], W, torch.float32)
        cond = BR.conditions(ref, free, W)
        if cond["gap"] and cond["f32"]:
            return cs, ref, R.decode(cs, cs["sd"], W, torch.float32, force=(ref["backptr"], ref["tokens"]))
    raise AssertionError("no gapped seed below %d" % limit)


@pytest.mark.parametrize("Bd", [1, 9, 17])
@pytest.mark.parametrize("W", [1, 3, 8])
def test_plain_entry_envelope(Bd, W):
    for max_len in (1, 5):
        cs, ref, chain = _gapped(lambda seed: _plain_problem(Bd, seed), W, max_len)
        for fast in (True, False):
            rc, got = _plain_call(cs, W, max_len, fast)
            assert rc == 0
            ok, fig = R.accept_decode(got, ref, chain, R.n_split(fast, fast, max_len))
            print("session beam envelope plain Bd=%d W=%d max_len=%d fast=%s: %s" % (Bd, W, max_len, fast, fig))
            assert ok, fig


def _cars_sub(B, SD):
    """the CARS golden's rows tiled to B sessions of SD + 1 queries: every source row, state and session row is one of the golden's"""
    cs = dict(R.load_case("cars", "full"))
    n_src, n_dec = cs["enc"].shape[0], cs["dec_h"].shape[0]
    src = torch.arange(B * (SD + 1)) % n_src
    dec = (torch.arange(B * SD) * 2) % n_dec
    flat = [a.reshape(n_src, -1) for a in cs["attns"]]
    cs.update(B=B, SD=SD, enc=cs["enc"][src], lens=cs["lens"][src], dec_h=cs["dec_h"][dec], dec_c=cs["dec_c"][dec],
              attns=[a[src].view(B, SD + 1, -1) for a in flat], session_cat=cs["session_cat"][src])
    return cs


@pytest.mark.parametrize("B,SD,W", [(1, 1, 8), (1, 1, 1), (17, 1, 3), (17, 1, 8)])
def test_cars_entry_envelope(cases, B, SD, W):
    m = cases["cars", "full", 4][1]
    base = _cars_sub(B, SD)
    for max_len in (1, 5):
        cs, ref, chain = _gapped(lambda seed: dict(base, sd=R.perturbed("cars", "full", W, seed=seed)), W, max_len)
        with torch.no_grad():
            m.token_prob_predictor2.weight.copy_(cs["sd"][R.PRED2].to(DEV))
        got = _decode(m, cs, W)
        ok, fig = R.accept_decode(got, ref, chain, R.n_split(True, True, max_len))
        print("session beam envelope cars Bd=%d W=%d max_len=%d: %s" % (B * SD, W, max_len, fig))
        assert ok, fig
    with torch.no_grad():
        m.token_prob_predictor2.weight.copy_(R.perturbed("cars", "full", 4)[R.PRED2].to(DEV))


def test_empty_batch_and_bad_arguments_on_the_device():
    cs = dict(_plain_problem(2, 1), max_len=3)
    for fast in (True, False):
        rc, out = _plain_call(cs, 3, 3, fast, rows=0)
        assert rc == 0 and all(bool((v == -7).all()) for v in out.values())      # nothing enqueued: every output as it was
    L = lib.load()
    BAD, WS = -1, -3
    p = lib.C.c_void_p(16)
    for W, VT in ((0, V_ENV), (9, V_ENV), (4, 3)):                                # width outside 1..8, VT < W
        assert L.nir_beam_plain_decode(p, p, 2, 32, p, 40, 8, p, p, p, p, p, p, VT, None, 2, 3, None, None, None, W, p, 1 << 30, p, p, p, None, None) == BAD
    assert L.nir_beam_plain_decode(None, p, 2, 32, p, 40, 8, p, p, p, p, p, p, 40, None, 2, 3, None, None, None, 3, p, 1 << 30, p, p, p, None, None) == BAD
    assert L.nir_beam_plain_decode(p, p, 2, 32, p, 40, 8, p, p, p, p, p, p, 40, None, 2, 3, None, None, None, 3, p, 64, p, p, p, None, None) == WS
