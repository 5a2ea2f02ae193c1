"""GPU (-m gpu): the HredQS beam search (csrc/beam.hip: nir_beam_hredqs_decode; HredQS.decode_beam; SessionRecommender.predict_session_nbest)
against the float64 restatement of tests/hredqs_beam_ref.py on the beam fixtures, in both forms of the entry; the two forms against each other;
bitwise repeatability; W = 1 against the greedy decode on the unmodified goldens; the C entry fed the recorded session states; B = 1 and S = 1;
eager against graph replay; and the n-best strings of a collated batch.

Which test reaches which kernel form: the fast form runs beam_gen_topk_kernel<BeamRowsSplit, 4, 4> on h64 / h96 / h256 at W <= 4, <4, 8> nowhere on the
fixtures (h64 has no W = 8 seed; the envelope module covers it), <2, 4> on h1024 at W <= 4 and <2, 8> on h1024 at W = 8 (48 beam rows: two
32-row blocks)."""
import pytest
import torch

import beam_ref as BR
import hredqs_beam_ref as R
import hredqs_ref as H
from conftest import T, load_golden
from context_attentive_ir_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = load_golden("hredqs")
VT = int(G["tgt_vocab"])
SPECIAL = ["<blank>", "<unk>", "<s>", "</s>"]
TGT_DICT = [SPECIAL[i] if i < 4 else "w%d" % i for i in range(VT)]
SRC_DICT = {TGT_DICT[i]: int(s) for i, s in enumerate(G["tgt2src"])}        # src_dict[tgt_dict[i]] = tgt2src[i]
CASE_W = R.case_w()
FORMS = ("fast", "plain")


def _wrap(tag, sd=None):
    from context_attentive_ir_amd.wrappers import SessionRecommender
    net = H.case(tag)[0]
    r = SessionRecommender(H.case_args(tag), SRC_DICT, TGT_DICT, net.state_dict())
    r.cuda()
    r.network.eval()
    if sd is not None:
        _set_bias(r.network, sd)
    return r


def _set_bias(net, sd):
    with torch.no_grad():
        net.generator.bias.copy_(sd["generator.bias"].to(DEV))


@pytest.fixture(scope="module")
def wrappers():
    """one wrapper on the GPU per case; a test sets the generator bias of its width"""
    return {tag: _wrap(tag) for tag in R.CASES}


@pytest.fixture(scope="module")
def refs():
    """every (case, W) once: (case, perturbed state dict, fp64 decode, fp32 decode forced along the fp64 choices, max_len)"""
    out = {}
    for tag, W in CASE_W:
        cs, sd, ml = R.load_case(tag), R.perturbed(tag, W), R.fixture_max_len(tag, W)
        ref = R.decode(cs, sd, W, max_len=ml)
        out[tag, W] = (cs, sd, ref, R.decode(cs, sd, W, torch.float32, force=(ref["backptr"], ref["tokens"]), max_len=ml), ml)
    return out


class _form(object):
    """`with _form(net, "plain")`: the entry's plain form (net.fast_decode = False), restored on exit; yields the weight struct"""

    def __init__(self, net, form):
        self.net, self.fast = net, form == "fast"

    def __enter__(self):
        self.net.fast_decode = self.fast
        w = self.net._decoder_weights().struct
        assert (bool(w.gen_frag), bool(w.rnn_whh_frag), bool(w.rnn_gate_fold)) == (self.fast,) * 3
        return w

    def __exit__(self, *exc):
        self.net.fast_decode = True
        return False


def _decode(net, cs, W, max_len):
    B, S = cs["B"], cs["S"]
    out = net.decode_beam(cs["src"].to(DEV), cs["lens"].to(DEV), max_len, W, tgt2src=cs["lut"].to(DEV), return_backptr=True)
    assert set(out) == {"predictions", "scores", "lengths", "backptr"}     # there are no attentions
    assert out["predictions"].shape == (B, S, W, max_len) and out["predictions"].dtype == torch.int64
    assert out["scores"].shape == (B, S, W) and out["scores"].dtype == torch.float32
    assert out["lengths"].shape == (B, S, W) and out["lengths"].dtype == torch.int64
    assert out["backptr"].shape == (max_len, B * S, W) and out["backptr"].dtype == torch.int32
    return out


def _same_bits(a, b):
    for k in ("predictions", "scores", "lengths", "backptr"):
        assert torch.equal(a[k], b[k]), k


def _flat(out, Bd):
    return dict(out, predictions=out["predictions"].reshape(Bd, *out["predictions"].shape[2:]), scores=out["scores"].reshape(Bd, -1),
                lengths=out["lengths"].reshape(Bd, -1))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tag,W", CASE_W)
def test_beam_decode_matches_the_fp64_restatement(wrappers, refs, tag, W, form):
    cs, sd, ref, chain, ml = refs[tag, W]
    net = wrappers[tag].network
    _set_bias(net, sd)
    with _form(net, form):
        got = _decode(net, cs, W, ml)
        again = _decode(net, cs, W, ml)
    ok, fig = R.accept_decode(_flat(got, cs["B"] * cs["S"]), ref, chain, R.n_split(cs["QL"], cs["S"], form == "fast", ml))
    print("hredqs beam bound %s W=%d %s: %s" % (tag, W, form, fig))
    assert ok, fig
    sc = got["scores"].reshape(-1, W).cpu()
    assert bool((sc[:, :-1] >= sc[:, 1:]).all())                                # best beam first
    _same_bits(again, got)                                                      # the same bits


@pytest.mark.parametrize("tag,W", [(t, W) for t, W in CASE_W if W in (4, 8)])
def test_fast_and_plain_forms_agree_in_every_token(wrappers, refs, tag, W):
    cs, sd, ref, chain, ml = refs[tag, W]
    net = wrappers[tag].network
    _set_bias(net, sd)
    out = {}
    for form in FORMS:
        with _form(net, form):
            out[form] = _decode(net, cs, W, ml)
    for k in ("predictions", "lengths", "backptr"):
        assert torch.equal(out["fast"][k], out["plain"][k]), k
    assert float((out["fast"]["scores"] - out["plain"]["scores"]).abs().max()) <= 1e-3


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tag", R.CASES)
def test_width_one_equals_the_greedy_decode_token_for_token(tag, form):
    cs = R.load_case(tag)
    net = _wrap(tag).network                                                    # the unmodified golden
    with _form(net, form):
        greedy = net.decode(cs["src"].to(DEV), cs["lens"].to(DEV), cs["max_len"], None, None, tgt2src=cs["lut"].to(DEV))["predictions"]
        beam = _decode(net, cs, 1, cs["max_len"])
    assert torch.equal(greedy.cpu(), cs["greedy"])
    pred, n = beam["predictions"][:, :, 0], beam["lengths"][:, :, 0]
    for b in range(cs["B"]):
        for s in range(cs["S"]):                                                # until a row emits EOS (the greedy decode goes on behind it)
            assert torch.equal(pred[b, s, :int(n[b, s])], greedy[b, s, :int(n[b, s])]), (b, s)
            assert bool((pred[b, s, int(n[b, s]):] == BR.EOS).all())
    assert bool((beam["backptr"] == 0).all())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tag,W", [("h64", 4), ("h1024", 8)])
def test_c_entry_on_the_recorded_states_equals_the_model_path(wrappers, refs, tag, W, form):
    """h_steps / c_steps are the reference's recorded session states (tests/golden/hredqs.npz: step-major), not the ones this library encodes"""
    cs, sd, ref, chain, ml = refs[tag, W]
    net = wrappers[tag].network
    _set_bias(net, sd)
    L = lib.load()
    B, S, Hs = cs["B"], cs["S"], cs["cfg"]["nhid_session"]
    g = H.case(tag)[2]
    hs, cs_ = (T(g[k]).view(S, B, Hs).transpose(0, 1).contiguous().to(DEV) for k in ("enc_h", "enc_c"))     # [B, S, H]
    with _form(net, form):
        model = _decode(net, cs, W, ml)
        w = net._decoder_weights()
        table = net.embedder.word_embeddings.table.detach().float().contiguous()
        lut = cs["lut"].to(DEV)
        out = {"predictions": torch.full((B, S, W, ml), -7, dtype=torch.int64, device=DEV), "scores": torch.full((B, S, W), -7.0, device=DEV),
               "lengths": torch.full((B, S, W), -7, dtype=torch.int64, device=DEV), "backptr": torch.full((ml, B * S, W), -7, dtype=torch.int32, device=DEV)}
        nb = L.nir_beam_hredqs_decode_workspace_bytes(B, S, W, ml, w.ref())
        assert nb > 0
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        for with_bp in (True, False):                                           # the workspace size covers a call without the caller's back-pointers
            lib.check(L.nir_beam_hredqs_decode(lib.ptr(hs), lib.ptr(cs_), B, S, lib.ptr(table), table.shape[0], table.shape[1], lib.ptr(lut), BR.BOS, ml,
                                               w.ref(), W, lib.ptr(ws), nb, lib.ptr(out["predictions"]), lib.ptr(out["scores"]), lib.ptr(out["lengths"]),
                                               lib.ptr(out["backptr"]) if with_bp else None, lib.stream()), "nir_beam_hredqs_decode")
            torch.cuda.synchronize()
            for k in ("predictions", "lengths", "backptr"):
                assert torch.equal(out[k], model[k]), (k, with_bp)
            assert float((out["scores"] - model["scores"]).abs().max()) <= 1e-3 * float(model["scores"].abs().max())
    ok, fig = R.accept_decode(_flat(out, B * S), ref, chain, R.n_split(cs["QL"], S, form == "fast", ml))
    print("hredqs beam bound %s W=%d %s on the recorded states: %s" % (tag, W, form, fig))
    assert ok, fig


def _gapped(tag, W, max_len, limit=100, **cut):
    """the first bias seed at which the cut-down batch keeps every float64 gap >= 1e-3 and the free float32 decode agrees -- decided on the CPU"""
    cs = R.sub_case(tag, **cut)
    for seed in range(1, limit):
        sd = R.perturbed(tag, W, seed=seed)
        ref = R.decode(cs, sd, W, max_len=max_len)
        cond = BR.conditions(ref, R.decode(cs, sd, W, torch.float32, max_len=max_len), W)
        if cond["gap"] and cond["f32"]:
            return cs, sd, ref, R.decode(cs, sd, W, torch.float32, force=(ref["backptr"], ref["tokens"]), max_len=max_len)
    raise AssertionError("no gapped seed below %d" % limit)


@pytest.mark.parametrize("tag", ["h96", "h1024"])
@pytest.mark.parametrize("cut", [dict(b=1), dict(s=2), dict(b=0, s=0)])
def test_single_session_and_single_query(wrappers, tag, cut):
    net = wrappers[tag].network
    W, ml = 4, 5
    cs, sd, ref, chain = _gapped(tag, W, ml, **cut)
    assert (cs["B"] == 1) == ("b" in cut) and (cs["S"] == 1) == ("s" in cut)
    _set_bias(net, sd)
    for form in FORMS:
        with _form(net, form):
            got = _decode(net, cs, W, ml)
        ok, fig = R.accept_decode(_flat(got, cs["B"] * cs["S"]), ref, chain, R.n_split(cs["QL"], cs["S"], form == "fast", ml))
        print("hredqs beam bound %s %s %s: %s" % (tag, cut, form, fig))
        assert ok, fig
    empty = net.decode_beam(cs["src"][:0].to(DEV), cs["lens"][:0].to(DEV), ml, W)
    assert empty["predictions"].shape == (0, cs["S"], W, ml) and empty["scores"].shape == (0, cs["S"], W)


# ---- the wrapper --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["h64", "h1024"])
def test_predict_session_nbest_eager_and_graph_replay(refs, tag):
    cs, sd, ref, chain, ml = refs[tag, 4]
    r = _wrap(tag, sd)
    assert r.args.max_query_len == ml
    ex = dict(source_words=cs["src"], source_lens=cs["lens"])
    ex2 = {k: v.roll(1, 0).contiguous() for k, v in ex.items()}                 # the same shape, other contents
    r.args.predict_graphs = False
    eager = [r.predict_session_nbest(e, 4) for e in (ex, ex2)]
    assert r._graphs is None or r._graphs.captures == 0
    r.args.predict_graphs = True
    r.predict_graph_min_calls = 2
    r.clear_predict_graphs()
    outs = [r.predict_session_nbest(ex, 4) for _ in range(3)] + [r.predict_session_nbest(ex2, 4)]      # eager, captured + replayed, replayed, other contents
    assert r._graphs is not None and r._graphs.captures == 1 and r._graphs.replays >= 3
    for o, want in zip(outs, [eager[0]] * 3 + [eager[1]]):
        assert set(o) == {"prediction_ids", "scores", "lengths"}
        assert o["prediction_ids"].shape == (cs["B"], cs["S"], 4, ml)
        for k in ("prediction_ids", "scores", "lengths"):
            assert torch.equal(o[k].cpu(), want[k].cpu()), k
    assert not torch.equal(eager[0]["scores"], eager[1]["scores"])             # (the two batches do differ)
    got = dict(predictions=eager[0]["prediction_ids"], scores=eager[0]["scores"], lengths=eager[0]["lengths"])
    ok, fig = R.accept_decode(_flat(got, cs["B"] * cs["S"]), ref, chain, R.n_split(cs["QL"], cs["S"], True, ml))   # through the dictionaries' table
    assert ok, fig
    r.predict_session_nbest(ex, 3)                                              # another width: a graph of its own, not a replay of W = 4's
    r.predict_session_nbest(ex, 3)
    assert r._graphs.captures == 2


def test_predict_session_nbest_returns_the_text_fields(refs):
    cs, sd, ref, chain, ml = refs["h64", 4]
    r = _wrap("h64", sd)
    B, S, W = cs["B"], cs["S"], 4
    lens = cs["lens"]
    toks = [[["<s>"] + ["s%d_%d_%d" % (b, s, j) for j in range(int(lens[b, s]))] + ["</s>"] for s in range(S)] for b in range(B)]
    tgts = [[["<s>", "t%d_%d" % (b, s), "x", "</s>"] for s in range(S)] for b in range(B)]
    ex = dict(source_words=cs["src"], source_lens=lens, ids=["q%d_" % b for b in range(B)], source_tokens=toks, target_tokens=tgts, src_vocab=None,
              session_len=S, batch_size=B)
    out, one = r.predict_session_nbest(ex, W), r.predict(ex)
    assert out["ex_ids"] == one["ex_ids"] and out["targets"] == one["targets"] and out["src_sequences"] == one["src_sequences"]
    ids = out["prediction_ids"].cpu()
    assert torch.equal(ids.reshape(B * S, W, ml), ref["predictions"])
    assert len(out["predictions"]) == B * S
    seen_eos = False
    for s in range(S):                                                          # step-major, like predict()
        for b in range(B):
            row = out["predictions"][s * B + b]
            assert len(row) == W
            for k in range(W):
                sent = []
                for wd in ids[b, s, k].tolist():
                    if wd == BR.BOS:
                        continue
                    if wd == BR.EOS:
                        seen_eos = True
                        break
                    sent.append(TGT_DICT[wd])
                assert row[k] == (" ".join(sent) if sent else "0")
    assert seen_eos                                                             # (the fixture ends some suggestions early)
