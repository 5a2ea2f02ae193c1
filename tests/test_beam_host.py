"""Host-side (no GPU) checks of the beam search: the restatement's state shuffle against the reference's recorded repeat_beam_size_times /
beam_update (tests/golden/beam_state.npz), W = 1 against the recorded greedy decodes, the search core against brute force, the conditions of
the beam fixtures (tests/golden/beam_seeds.json), the teeth of the acceptance criterion, the wrappers' refusals and the registration of the
new symbols."""
import os
import re

import pytest
import torch

import beam_ref as R
import gemm_ref
import gru_dec_ref as GR
import seq2seq_ref as S
from conftest import ROOT, T, load_golden

SRC, LENS, MAXLEN = R.inputs()
CASE_W = [(k, t, W) for k, t in R.CASES for W in R.widths(k, t)]


@pytest.fixture(scope="module")
def decodes():
    """per (kind, tag, W): (state dict, cfg, cell, lut, fp64 decode, free fp32 decode, fp32 decode forced along the fp64 choices) -- once"""
    out = {}
    for kind, tag, W in CASE_W:
        net, c, cell, lut = R.case(kind, tag, W)
        sd = net.state_dict()
        ref = R.decode(sd, c, cell, SRC, LENS, MAXLEN, W, lut)
        free = R.decode(sd, c, cell, SRC, LENS, MAXLEN, W, lut, torch.float32)
        chain = R.decode(sd, c, cell, SRC, LENS, MAXLEN, W, lut, torch.float32, force=(ref["backptr"], ref["tokens"]))
        out[kind, tag, W] = (sd, c, cell, lut, ref, free, chain)
    return out


# ---- the state shuffle is the reference's ---------------------------------------------------------------------------------------------------
def test_repeat_and_reorder_equal_the_references_state_helpers():
    g = load_golden("beam_state")
    pos = T(g["positions"])
    B, W = pos.shape
    for names in (("lstm_h", "lstm_c"), ("gru_h",)):
        state = tuple(T(g[n])[0] for n in names)
        rep = R.repeat_state(state, W)
        upd = R.reorder_state(tuple(T(g["pre_" + n])[0] for n in names), pos)
        for n, r, u in zip(names, rep, upd):
            assert torch.equal(r, T(g["rep_" + n])[0]) and torch.equal(u, T(g["upd_" + n])[0]), n
    # the layout is k B + b, and the fixture's permutations are not the identity
    assert torch.equal(T(g["rep_gru_h"])[0, 2 * B + 1], T(g["gru_h"])[0, 1])
    assert all(pos[b].tolist() != list(range(W)) for b in range(B))
    assert not torch.equal(T(g["upd_gru_h"]), T(g["pre_gru_h"]))


# ---- W = 1 ties the search to the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", [("s2s", t) for t in S.CASES] + [("gru", t) for t in GR.S2S_CASES])
def test_width_one_reproduces_the_recorded_greedy_decode(kind, tag):
    net, c, g = S.case(tag) if kind == "s2s" else GR.case("s2s", tag)
    out = R.decode(net.state_dict(), c, "LSTM" if kind == "s2s" else "GRU", SRC, LENS, MAXLEN, 1, T(g["tgt2src"]))
    assert torch.equal(out["predictions"][:, 0], T(g["predictions"]))
    assert not bool((out["predictions"] == R.EOS).any())                     # (the greedy fixtures never emit EOS: every step is compared)
    assert float((out["attentions"][:, 0] - S.pad_attn(g["attentions"], SRC.shape[1]).double()).abs().max()) <= 1e-6
    assert torch.equal(out["lengths"], torch.full_like(out["lengths"], MAXLEN))


# ---- the search core against brute force ------------------------------------------------------------------------------------------------------
def _core(table, W, max_len, fault=None):
    state0 = (torch.zeros(1, 1, dtype=table.dtype),)
    return R.search(R.table_step(table), state0, 1, W, max_len, fault=fault, bos=table.shape[1])


def test_search_core_equals_brute_force():
    from context_attentive_ir_amd.detinit import det_tensor
    table = 2.0 * det_tensor("beam.table", (5, 4), 7, scale=1.0).double()
    want = R.brute_force(table, 3)
    assert len(want) == 40                                                   # 27 + 9 + 3 + 1 EOS-collapsed sequences
    got = _core(table, 16, 3)
    for j in range(16):
        assert tuple(got["predictions"][0, j].tolist()) == want[j][1], j
        assert abs(float(got["scores"][0, j]) - want[j][0]) <= 1e-12
    assert got["lengths"][0].tolist() == [(list(w[1]).index(R.EOS) + 1) if R.EOS in w[1] else 3 for w in want[:16]]
    # a narrow beam is a prefix-consistent subset: its best sequence is never better than the exhaustive best
    narrow = _core(table, 2, 3)
    assert float(narrow["scores"][0, 0]) <= want[0][0] + 1e-12


def test_search_core_tie_rule_on_an_exactly_tied_table():
    table = torch.zeros(5, 4, dtype=torch.float64)                           # every continuation of a live beam ties: k VT + v ascending decides
    want = sorted(R.brute_force(table, 3), key=lambda x: (-x[0], x[1]))
    got = _core(table, 16, 3)
    assert [tuple(r) for r in got["predictions"][0].tolist()] == [w[1] for w in want[:16]]
    assert float(got["gaps"].min()) == 0.0
    bad = _core(table, 16, 3, fault="tie_last")
    assert not torch.equal(bad["predictions"], got["predictions"]) or not torch.equal(bad["backptr"], got["backptr"])


# ---- the beam fixtures ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag,W", CASE_W)
def test_fixture_conditions_hold_at_every_step(decodes, kind, tag, W):
    sd, c, cell, lut, ref, free, chain = decodes[kind, tag, W]
    cond = R.conditions(ref, free, W)
    print("beam fixture %s %s W=%d: %s" % (kind, tag, W, cond))
    assert ref["gaps"].shape == (MAXLEN, SRC.shape[0], W)                    # no step and no source row is left out
    assert cond["gap"] and cond["f32"], cond
    if W > 1:
        assert cond["eos"] and cond["mixed"] and cond["moved"], cond
    assert torch.equal(chain["predictions"], ref["predictions"])
    ok, fig = R.accept_decode(dict(chain, backptr=chain["backptr"]), ref, chain, 0)
    assert ok, fig


@pytest.mark.parametrize("kind,tag", R.CASES)
@pytest.mark.parametrize("fault", ["no_reorder", "raw_logit", "eos_grows", "all_live_step0"])       # (tie_last: the tied table above)
def test_the_criterion_rejects_every_planted_fault_at_the_margins_cap(decodes, kind, tag, fault):
    sd, c, cell, lut, ref, free, chain = decodes[kind, tag, 4]
    bad = R.decode(sd, c, cell, SRC, LENS, MAXLEN, 4, lut, fault=fault)
    ok, fig = R.accept_decode(bad, ref, chain, 2 * MAXLEN, margin=gemm_ref.MARGIN_CAP)
    assert not ok, (kind, tag, fault, fig)


# ---- wrappers -----------------------------------------------------------------------------------------------------------------------------------
def test_only_the_seq2seq_wrappers_have_a_beam():
    import context_attentive_ir_amd.wrappers as Wr
    from context_attentive_ir_amd.config import default_args
    kw = dict(src_vocab_size=50, tgt_vocab_size=50, nhid=32, nlayers=1)
    c = Wr.CopyRecommender(default_args("ACG", copy_attn=True, **kw), list(range(50)), list(range(50)))
    with pytest.raises(NotImplementedError, match="beam"):
        c.predict_beam({}, 4)
    s = Wr.SessionRecommender(default_args("HREDQS", bidirection=False, **kw))
    with pytest.raises(NotImplementedError, match="beam"):
        s.predict_beam({}, 4)
    r = Wr.Recommender(default_args("SEQ2SEQ", **kw))
    assert r.network.fuse_generator_topk is True and not hasattr(r.args, "beam_size")
    r.network.eval()
    with pytest.raises(RuntimeError, match="ROCm device only"):            # no CPU fallback
        r.network.decode_beam(SRC % 50, LENS, MAXLEN, 4)


# ---- symbols and arguments ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exist_with_their_prototypes():
    from context_attentive_ir_amd import lib
    C = lib.C
    names = {"nir_beam_gen_topk_workspace_bytes", "nir_beam_gen_topk", "nir_beam_select", "nir_beam_reorder",
             "nir_beam_seq2seq_decode_workspace_bytes", "nir_beam_seq2seq_decode", "nir_beam_seq2seq_gru_decode_workspace_bytes",
             "nir_beam_seq2seq_gru_decode"}
    main = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    assert '#include "neuroir_beam.h"' in main and not re.findall(r"\bnir_beam_[a-z0-9_]*\s*\(", main)
    hdr = open(os.path.join(ROOT, "include", "neuroir_beam.h")).read()
    declared = set(re.findall(r"\b(nir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert names == declared == set(lib.BEAM_SIGNATURES) and not names & (set(lib.SIGNATURES) | set(lib.GRU_DECODE_SIGNATURES))
    assert all(n.startswith("nir_beam_") for n in names)
    L = lib.load()
    for n in names:
        assert hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, hdr, re.S)
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert nargs == len(lib.BEAM_SIGNATURES[n][1]), n
    assert "decoders/state.py:16-31" in hdr and ":65-69" in hdr                # the reference lines the layout comes from
    assert lib.BEAM_MAX_W == 8 and lib.BEAM_EOS == 3
    # bad arguments are refused before anything is enqueued (no device needed)
    err = lambda: L.nir_last_error_string()                                  # noqa: E731
    p = C.c_void_p(16)
    big = 1 << 30
    assert L.nir_beam_gen_topk_workspace_bytes(4, 96, 10, 3, 0) == 4 * 10 * 4 + 256
    assert L.nir_beam_gen_topk_workspace_bytes(4, 96, 10, 9, 0) == 0 and L.nir_beam_gen_topk_workspace_bytes(4, 96, 2, 3, 0) == 0
    assert L.nir_beam_gen_topk_workspace_bytes(4, 48, 10, 3, 1) == 0          # K = 48 has no fused form
    for W, VT in ((0, 10), (9, 10), (4, 3)):
        assert L.nir_beam_gen_topk(p, 2, 96, p, p, None, VT, W, p, big, p, p, p, None) == -1 and b"beam width" in err()
        assert L.nir_beam_select(p, p, p, 2, W, VT, None, 10, p, p, p, p, p, None) == -1 and b"beam width" in err()
    assert L.nir_beam_gen_topk(None, 2, 96, p, p, None, 10, 3, p, big, p, p, p, None) == -1 and b"null" in err()
    assert L.nir_beam_gen_topk(p, 2, 96, p, p, None, 10, 3, p, 16, p, p, p, None) == -3 and b"workspace" in err()
    assert L.nir_beam_gen_topk(p, 0, 96, p, p, None, 10, 3, p, 16, p, p, p, None) == 0
    assert L.nir_beam_select(p, p, None, 2, 3, 10, None, 10, p, p, p, p, p, None) == -1 and b"null" in err()
    assert L.nir_beam_reorder(None, 2, 3, 8, p, p, None, None, None, None, None) == -1 and b"null" in err()
    assert L.nir_beam_reorder(p, 2, 9, 8, p, C.c_void_p(32), None, None, None, None, None) == -1 and b"beam width" in err()
    assert L.nir_beam_reorder(p, 2, 3, 8, p, p, None, None, None, None, None) == -1 and b"aliases" in err()
    assert L.nir_beam_reorder(p, 2, 3, 6, p, C.c_void_p(32), None, None, None, None, None) == -1 and b"bad dims" in err()
    w = lib.Seq2seqDecoderWeights()
    for f in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "attn_out_w", "gen_w", "gen_b"):
        setattr(w, f, 16)
    w.H, w.attn_type, w.VT = 8, lib.S2S_ATTN["dot"], 10
    ref = C.byref(w)
    for fn, state in ((L.nir_beam_seq2seq_decode, [p, p]), (L.nir_beam_seq2seq_gru_decode, [p])):
        tail = [p, 20, 4, None, 2, 6, ref, p]
        for W in (0, 9, 11):
            assert fn(*state, p, p, 2, 7, W, *tail, big, p, p, p, p, None, None) == -1 and b"beam width" in err()
        assert fn(*state, p, p, 2, 7, 3, *tail, 16, p, p, p, p, None, None) == -3 and b"workspace" in err()
        assert fn(*state, p, p, 2, 7, 3, *tail, big, None, p, p, p, None, None) == -1 and b"null" in err()
        assert fn(*state, p, p, 0, 7, 3, *tail, big, p, p, p, p, None, None) == 0
    assert L.nir_beam_seq2seq_decode_workspace_bytes(2, 7, 3, 6, ref) > 0 and L.nir_beam_seq2seq_decode_workspace_bytes(2, 7, 9, 6, ref) == 0


@pytest.mark.parametrize("packs", ["generator", "generator+step"])
def test_an_empty_batch_is_accepted_in_the_fused_forms_too(packs):
    """B = 0 with the generator fragment given (H a multiple of 32: the fused top-k is chosen) enqueues nothing and needs no device -- the
    partials are sized per row block, and there is none; with the step's packs too the fp16 term pairs join the workspace"""
    from context_attentive_ir_amd import lib
    C = lib.C
    L = lib.load()
    p = C.c_void_p(16)
    w = lib.Seq2seqDecoderWeights()
    for f in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "attn_out_w", "gen_w", "gen_b", "gen_frag"):
        setattr(w, f, 16)
    if packs == "generator+step":
        w.rnn_gate_fold = w.rnn_whh_frag = 16
    w.H, w.attn_type, w.VT = 32, lib.S2S_ATTN["dot"], 100
    ref = C.byref(w)
    tail = [p, 20, 4, None, 2, 6, ref, p]
    for name, state in (("nir_beam_seq2seq_decode", [p, p]), ("nir_beam_seq2seq_gru_decode", [p])):
        fn, size = getattr(L, name), getattr(L, name + "_workspace_bytes")
        empty = size(0, 7, 3, 6, ref)
        assert empty < size(2, 7, 3, 6, ref)                                   # (no rows: nothing to hold)
        assert fn(*state, p, p, 0, 7, 3, *tail, 1 << 30, p, p, p, p, None, None) == 0
        assert fn(*state, p, p, 0, 7, 3, *tail, 1 << 30, p, p, p, p, p, None) == 0          # with the caller's back-pointers
        assert fn(*state, p, p, 0, 7, 9, *tail, 1 << 30, p, p, p, p, None, None) == -1
    assert L.nir_beam_gen_topk_workspace_bytes(0, 32, 100, 3, 1) == 0
    assert L.nir_beam_gen_topk(p, 0, 32, p, p, p, 100, 3, p, 16, p, p, p, None) == 0
    # the term pairs are part of the workspace only when the fp16-term step runs
    w.rnn_gate_fold = w.rnn_whh_frag = None
    small = L.nir_beam_seq2seq_decode_workspace_bytes(4, 7, 3, 6, ref)
    w.rnn_gate_fold = w.rnn_whh_frag = 16
    assert L.nir_beam_seq2seq_decode_workspace_bytes(4, 7, 3, 6, ref) > small
    assert L.nir_beam_seq2seq_gru_decode_workspace_bytes(2, 7, 3, 6, ref) > 0
