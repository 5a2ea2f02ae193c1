"""Host-side (no GPU) checks of the session models' beam search: the restatement at W = 1 against the recorded greedy decodes of the unmodified
goldens, the conditions of the beam fixtures (tests/golden/session_beam_seeds.json), the teeth of the acceptance criterion (beam_ref's four
model-independent faults and the two that only the session layout can make), the registration of the new symbols and the Python surface."""
import os
import re

import pytest
import torch

import gemm_ref
import session_beam_ref as R

CASE_W = [(k, t, W) for k, t in R.CASES for W in R.widths(k, t)]


@pytest.fixture(scope="module")
def decodes():
    """per (kind, tag, W): (case, perturbed state dict, fp64 decode, free fp32 decode, fp32 decode forced along the fp64 choices) -- once"""
    out = {}
    for kind, tag, W in CASE_W:
        cs, sd = R.load_case(kind, tag), R.perturbed(kind, tag, W)
        ref = R.decode(cs, sd, W)
        free = R.decode(cs, sd, W, torch.float32)
        chain = R.decode(cs, sd, W, torch.float32, force=(ref["backptr"], ref["tokens"]))
        out[kind, tag, W] = (cs, sd, ref, free, chain)
    return out


# ---- W = 1 ties the restatement to the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", R.CASES)
def test_width_one_reproduces_the_recorded_greedy_decode(kind, tag):
    cs = R.load_case(kind, tag)
    out = R.decode(cs, cs["sd"], 1)
    pred, want = out["predictions"][:, 0], cs["greedy"]
    assert pred.shape == want.shape
    for i in range(want.shape[0]):                                              # up to each row's first EOS
        n = int(out["lengths"][i, 0])
        assert torch.equal(pred[i, :n], want[i, :n]), (kind, tag, i)
    assert int(out["lengths"].min()) >= 1


# ---- the beam fixtures ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag,W", CASE_W)
def test_fixture_conditions_hold_at_every_step(decodes, kind, tag, W):
    cs, sd, ref, free, chain = decodes[kind, tag, W]
    cond = R.conditions(cs, sd, ref, free, W)
    print("session beam fixture %s W=%d: %s" % (R.name(kind, tag), W, cond))
    Bd = cs["B"] * cs["SD"]
    assert ref["gaps"].shape == (cs["max_len"], Bd, W)                          # no step and no source row is left out
    assert cond["gap"] and cond["f32"], cond
    if W > 1:
        assert cond["eos"] and cond["mixed"] and cond["moved"], cond
        assert abs(cond["min_gap"] - R.seeds()[R.name(kind, tag)][str(W)][1]) <= 1e-9       # the recorded smallest gap
    assert R.conditions_ok(cond, W), cond
    assert torch.equal(chain["predictions"], ref["predictions"])
    ok, fig = R.accept_decode(dict(chain), ref, chain, 0)
    assert ok, fig


def test_the_widest_case_crosses_the_generator_kernels_row_block():
    cs = R.load_case("cars", "full")
    assert cs["B"] * cs["SD"] == 9 and 8 in R.widths("cars", "full")          # 72 beam rows: more than one 64-row block of beam_gen_topk_kernel


@pytest.mark.parametrize("kind,tag", R.CASES)
@pytest.mark.parametrize("fault", ["no_reorder", "raw_logit", "eos_grows", "all_live_step0"])
def test_the_criterion_rejects_every_model_independent_fault_at_the_margins_cap(decodes, kind, tag, fault):
    cs, sd, ref, free, chain = decodes[kind, tag, 4]
    bad = R.decode(cs, sd, 4, fault=fault)
    ok, fig = R.accept_decode(bad, ref, chain, 2 * cs["max_len"], margin=gemm_ref.MARGIN_CAP)
    assert not ok, (kind, tag, fault, fig)


@pytest.mark.parametrize("tag,fault", [("full", "wrong_source_row"), ("full", "sess_dropped"), ("qoff", "sess_dropped"), ("doff", "sess_dropped")])
def test_the_criterion_rejects_the_session_layouts_faults_at_the_margins_cap(decodes, tag, fault):
    cs, sd, ref, free, chain = decodes["cars", tag, 4]
    assert cs["session_cat"] is not None                                        # KS > 0
    bad = R.decode(cs, sd, 4, fault=fault)
    ok, fig = R.accept_decode(bad, ref, chain, 2 * cs["max_len"], margin=gemm_ref.MARGIN_CAP)
    assert not ok, (tag, fault, fig)


# ---- symbols and arguments ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exist_with_their_prototypes():
    from conftest import ROOT
    from context_attentive_ir_amd import lib
    C = lib.C
    names = {"nir_beam_cars_decode_workspace_bytes", "nir_beam_cars_decode", "nir_beam_plain_decode_workspace_bytes", "nir_beam_plain_decode"}
    main = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    assert '#include "neuroir_session_beam.h"' in main
    hdr = open(os.path.join(ROOT, "include", "neuroir_session_beam.h")).read()
    declared = set(re.findall(r"\b(nir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert names == declared == set(lib.SESSION_BEAM_SIGNATURES)
    assert not names & (set(lib.SIGNATURES) | set(lib.GRU_DECODE_SIGNATURES) | set(lib.BEAM_SIGNATURES))
    L = lib.load()
    for n in names:
        assert hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, hdr, re.S)
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert nargs == len(lib.SESSION_BEAM_SIGNATURES[n][1]), n
    # bad arguments are refused before anything is enqueued (no device needed)
    err = lambda: L.nir_last_error_string()                                  # noqa: E731
    p = C.c_void_p(16)
    big = 1 << 30
    plain = lambda Bd, W, VT, ws, pred=p, H=8: L.nir_beam_plain_decode(p, p, Bd, H, p, 20, 4, p, p, p, p, p, p, VT, None, 2, 6, None, None, None, W, p, ws,   # noqa: E731
                                                                       pred, p, p, None, None)
    for W, VT in ((0, 10), (9, 10), (4, 3)):
        assert plain(2, W, VT, big) == -1 and b"beam width" in err()
        assert L.nir_beam_plain_decode_workspace_bytes(2, 8, VT, W, 6, 0, 0) == 0
    assert plain(2, 3, 10, big, pred=None) == -1 and b"null" in err()
    assert plain(2, 3, 10, big, H=6) == -1 and b"bad dims" in err()
    assert plain(2, 3, 10, 16) == -3 and b"workspace" in err()
    assert plain(0, 3, 10, big) == 0
    assert L.nir_beam_plain_decode_workspace_bytes(2, 8, 10, 3, 6, 0, 0) > L.nir_beam_plain_decode_workspace_bytes(0, 8, 10, 3, 6, 0, 0)
    assert L.nir_beam_plain_decode_workspace_bytes(2, 32, 100, 3, 6, 1, 0) > L.nir_beam_plain_decode_workspace_bytes(2, 32, 100, 3, 6, 0, 0)
    w = lib.CarsDecoderWeights()
    for f in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "attn_in_w", "attn_out_w", "dec_attn_w", "pred1_w", "pred2_w", "sess_w"):
        setattr(w, f, 16)
    w.HD, w.DQ, w.P, w.KS, w.VT = 8, 8, 8, 4, 10
    ref = C.byref(w)
    cars = lambda Bd, W, ws, pred=p, frag=None: L.nir_beam_cars_decode(p, p, p, p, 3, 5, p, Bd, p, p, 20, 4, None, 2, 6, ref, frag, W, p, ws, pred, p, p,   # noqa: E731
                                                                       None, None)
    for W in (0, 9, 11):
        assert cars(2, W, big) == -1 and b"beam width" in err()
    assert cars(2, 3, big, pred=None) == -1 and b"null" in err()
    assert cars(2, 3, 16) == -3 and b"workspace" in err()
    assert cars(0, 3, big) == 0 and cars(0, 3, big, frag=p) == 0
    assert L.nir_beam_cars_decode_workspace_bytes(3, 2, 5, 3, 6, ref, 0) > 0 and L.nir_beam_cars_decode_workspace_bytes(3, 2, 5, 9, 6, ref, 0) == 0
    w.P = 6
    assert cars(2, 3, big) == -1 and b"bad dims" in err()


def test_an_empty_batch_is_accepted_in_the_fused_forms_too():
    """Bd = 0 with the generator fragment and the step's packs given enqueues nothing and needs no device"""
    from context_attentive_ir_amd import lib
    C = lib.C
    L = lib.load()
    p = C.c_void_p(16)
    assert L.nir_beam_plain_decode(p, p, 0, 32, p, 20, 4, p, p, p, p, p, p, 100, None, 2, 6, p, p, p, 3, p, 1 << 30, p, p, p, p, None) == 0
    w = lib.CarsDecoderWeights()
    for f in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "attn_in_w", "attn_out_w", "dec_attn_w", "pred1_w", "pred2_w", "sess_w", "rnn_gate_fold",
              "rnn_whh_frag", "attn_q_w"):
        setattr(w, f, 16)
    w.HD, w.DQ, w.P, w.KS, w.VT = 32, 32, 32, 4, 100
    assert L.nir_beam_cars_decode(p, p, p, p, 3, 5, p, 0, p, p, 20, 4, None, 2, 6, C.byref(w), p, 3, p, 1 << 30, p, p, p, p, None) == 0
    assert L.nir_beam_cars_decode_workspace_bytes(3, 0, 5, 3, 6, C.byref(w), 1) < L.nir_beam_cars_decode_workspace_bytes(3, 2, 5, 3, 6, C.byref(w), 1)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------------
def test_the_session_models_and_their_wrapper_have_a_beam():
    import context_attentive_ir_amd.wrappers as Wr
    from context_attentive_ir_amd import multitask as M
    assert callable(getattr(Wr.Multitask, "predict_beam"))
    for cls in (M.CARS, M.M_MATCH_TENSOR, M.MNSRF):
        assert callable(getattr(cls, "decode_beam")), cls
    for kind, tag in (("cars", "full"), ("mmt", ""), ("mnsrf", "")):
        cs = R.load_case(kind, tag)
        from helpers import build_model
        if kind == "cars":
            from conftest import load_golden
            m = build_model("CARS", tgt_vocab_size=int(load_golden("cars_decode")["meta_vocab"]))
            kw = dict(encoded_source=cs["enc"], source_len=cs["lens"], session_attns=cs["attns"])
        else:
            m = build_model("M_MATCH_TENSOR" if kind == "mmt" else "MNSRF", tgt_vocab_size=cs["lut"].shape[0])
            kw = {}
        assert m.fuse_generator_topk is True
        with pytest.raises(RuntimeError, match="ROCm device only"):            # no CPU fallback
            m.decode_beam(states=(cs["dec_h"].unsqueeze(0), cs["dec_c"].unsqueeze(0)), max_len=cs["max_len"], beam_size=4, src_dict=None, tgt_dict=None,
                          batch_size=cs["B"], session_len=cs["SD"], **kw)
    from context_attentive_ir_amd.config import default_args
    w = Wr.Multitask(default_args("MNSRF", src_vocab_size=50, tgt_vocab_size=50))
    assert not hasattr(w.args, "beam_size")
    with pytest.raises(ValueError, match="beam_size"):
        w.predict_beam({}, 9)
