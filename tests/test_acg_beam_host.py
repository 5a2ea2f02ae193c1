"""Host-side (no GPU) checks of ACG's beam search: the search core of tests/acg_beam_ref.py against brute force, W = 1 against the recorded greedy
decodes of acg.npz, the conditions of the fixtures (tests/golden/acg_beam_seeds.json), the teeth of the acceptance criterion, the registration
of the new symbols and the refusals that need no device."""
import os
import re

import pytest
import torch

import acg_beam_ref as R
import acg_ref as AR
from conftest import ROOT, T

D = R.batch()
SRC, LENS, VT = D["src"], D["lens"], len(D["tgt_dict"])
CASE_W = [(k, t, W) for k, t in R.CASES for W in R.widths(k, t)]


def _decode(sd, c, cell, W, **kw):
    return R.decode(sd, c, cell, SRC, LENS, kw.pop("max_len", R.max_len(W)), W, D["idx"], D["e2t"], D["e2s"], **kw)


@pytest.fixture(scope="module")
def decodes():
    """per (kind, tag, W): (state dict, cfg, cell, fp64 decode, free fp32 decode, fp32 decode forced along the fp64 choices) -- once"""
    out = {}
    for kind, tag, W in CASE_W:
        net, c, cell = R.case(kind, tag, W)
        sd = net.state_dict()
        ref = _decode(sd, c, cell, W)
        free = _decode(sd, c, cell, W, dtype=torch.float32)
        chain = _decode(sd, c, cell, W, dtype=torch.float32, force=(ref["backptr"], ref["tokens"]))
        out[kind, tag, W] = (sd, c, cell, ref, free, chain)
    return out


# ---- the search core against brute force ------------------------------------------------------------------------------------------------------
NV, NC = 4, 3                                                                # VT 4, CV 3: extended ids 0..6, slot 2 (id 6) collapsed: no candidate


def _table(tied=False):
    from context_attentive_ir_amd.detinit import det_tensor
    N = NV + NC
    raw = torch.zeros(N + 1, N, dtype=torch.float64) if tied else 2.0 * det_tensor("acg_beam.table", (N + 1, N), 11, scale=1.0).double()
    live = torch.ones(N + 1, N, dtype=torch.bool)
    live[:, N - 1] = False
    logp = torch.log_softmax(raw.masked_fill(~live, float("-inf")), 1)         # a distribution over the live ids; the dead one holds -inf
    return logp, live


def _core(logp, live, W, max_len, fault=None):
    N = logp.shape[1]
    state0 = (torch.zeros(1, 1, dtype=logp.dtype),)
    return R.search(R.table_step(logp, live), state0, 1, W, max_len, lambda b, k, e: e, fault=fault, bos=N)


def test_search_core_equals_brute_force():
    logp, live = _table()
    want = R.brute_force(logp, live, 3)
    assert len(want) == 156                                                  # 5^3 + 5^2 + 5 + 1 EOS-collapsed sequences over 6 live ids
    got = _core(logp, live, 216, 3)                                          # wide enough to prune nothing
    for j in range(len(want)):
        assert tuple(got["predictions"][0, j].tolist()) == want[j][1], j
        assert abs(float(got["scores"][0, j]) - want[j][0]) <= 1e-12
    assert NV + NC - 1 not in got["predictions"][0, :len(want)].unique().tolist()          # the collapsed slot is never offered
    assert got["lengths"][0, :len(want)].tolist() == [(list(w[1]).index(R.EOS) + 1) if R.EOS in w[1] else 3 for w in want]
    narrow = _core(logp, live, 2, 3)
    assert float(narrow["scores"][0, 0]) <= want[0][0] + 1e-12


def test_search_core_tie_rule_on_an_exactly_tied_table():
    logp, live = _table(tied=True)                                           # every continuation of a live beam ties: k (VT + CV) + e ascending decides
    want = sorted(R.brute_force(logp, live, 3), key=lambda x: (-x[0], x[1]))
    got = _core(logp, live, 216, 3)
    assert [tuple(r) for r in got["predictions"][0, :len(want)].tolist()] == [w[1] for w in want]
    assert float(got["gaps"].min()) == 0.0


# ---- W = 1 ties the search to the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", AR.CASES)
def test_width_one_reproduces_the_recorded_greedy_decode(tag):
    net, c, g = AR.case(tag)
    out = _decode(net.state_dict(), c, "LSTM", 1, max_len=int(AR.golden()["max_len"]))
    assert torch.equal(out["predictions"][:, 0], T(g["predictions"]))


# ---- the beam fixtures ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag,W", CASE_W)
def test_fixture_conditions_hold_at_every_step(decodes, kind, tag, W):
    sd, c, cell, ref, free, chain = decodes[kind, tag, W]
    cond = R.conditions(ref, free, W, VT, D["e2t"])
    print("acg beam fixture %s %s W=%d: %s" % (kind, tag, W, cond))
    assert ref["gaps"].shape == (R.max_len(W), SRC.shape[0], W)              # no step and no source row is left out
    assert cond["gap"] and cond["f32"], cond
    if W > 1:
        assert cond["eos"] and cond["mixed"] and cond["moved"] and cond["slot"] and cond["fed"], cond
    assert torch.equal(chain["predictions"], ref["predictions"])
    ok, fig = R.accept_decode(dict(chain, backptr=chain["backptr"]), ref, chain, 0)
    assert ok, fig


@pytest.mark.parametrize("kind,tag", R.CASES)
@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_criterion_rejects_every_planted_fault_at_the_margins_cap(decodes, kind, tag, fault):
    sd, c, cell, ref, free, chain = decodes[kind, tag, 4]
    bad = _decode(sd, c, cell, 4, fault=fault)
    ok, fig = R.accept_decode(bad, ref, chain, 2 * R.max_len(4), margin=R.MARGIN_CAP)
    assert not ok, (kind, tag, fault, fig)


# ---- symbols and arguments ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exist_with_their_prototypes():
    from context_attentive_ir_amd import lib
    C = lib.C
    names = {"nir_acg_beam_gen_select_workspace_bytes", "nir_acg_beam_gen_select", "nir_acg_beam_select", "nir_acg_beam_decode_workspace_bytes",
             "nir_acg_beam_decode", "nir_acg_beam_gru_decode_workspace_bytes", "nir_acg_beam_gru_decode"}
    main = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    assert '#include "neuroir_acg_beam.h"' in main and not re.findall(r"\bnir_acg_beam_[a-z0-9_]*\s*\(", main)
    hdr = open(os.path.join(ROOT, "include", "neuroir_acg_beam.h")).read()
    declared = set(re.findall(r"\b(nir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    others = set(lib.SIGNATURES) | set(lib.GRU_DECODE_SIGNATURES) | set(lib.BEAM_SIGNATURES) | set(lib.SESSION_BEAM_SIGNATURES)
    assert names == declared == set(lib.ACG_BEAM_SIGNATURES) and not names & others
    L = lib.load()
    for n in names:
        assert hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, hdr, re.S)
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert nargs == len(lib.ACG_BEAM_SIGNATURES[n][1]), n
    assert "NOT a candidate" in hdr and "1e-10" in hdr                          # the header says what happens to a collapsed slot
    # bad arguments are refused before anything is enqueued (no device needed)
    err = lambda: L.nir_last_error_string()                                  # noqa: E731
    p = C.c_void_p(16)
    big = 1 << 30

    def gen(o=p, rows=2, VT=10, W=3, QL=7, CV=5, bytes_=big):
        return L.nir_acg_beam_gen_select(o, rows, 1, 96, p, p, None, VT, W, p, p, p, QL, p, QL, p, p, p, CV, p, bytes_, p, p, None)
    assert L.nir_acg_beam_gen_select_workspace_bytes(4, 96, 10, 3, 0) > 4 * 10 * 4
    assert L.nir_acg_beam_gen_select_workspace_bytes(4, 96, 10, 9, 0) == 0 and L.nir_acg_beam_gen_select_workspace_bytes(4, 96, 2, 3, 0) == 0
    assert L.nir_acg_beam_gen_select_workspace_bytes(4, 48, 10, 3, 1) == 0    # K = 48 has no fused form
    for W, vt in ((0, 10), (9, 10), (4, 3)):
        assert gen(W=W, VT=vt) == -1 and b"beam width" in err()
        assert L.nir_acg_beam_select(p, p, None, 2, W, vt, 5, None, p, 10, p, p, p, p, p, None) == -1 and b"beam width" in err()
    for QL, CV in ((0, 5), (4097, 5), (7, 1), (7, 1025)):
        assert gen(QL=QL, CV=CV) == -1 and b"outside" in err()
    assert L.nir_acg_beam_select(p, p, None, 2, 3, 10, 1, None, p, 10, p, p, p, p, p, None) == -1 and b"CV outside" in err()
    assert gen(o=None) == -1 and b"null" in err()
    assert L.nir_acg_beam_select(p, p, None, 2, 3, 10, 5, None, None, 10, p, p, p, p, p, None) == -1 and b"null" in err()
    assert gen(bytes_=16) == -3 and b"workspace" in err()
    assert gen(rows=0, bytes_=16) == 0
    assert L.nir_acg_beam_select(p, p, None, 0, 3, 10, 5, None, p, 10, p, p, p, p, p, None) == 0
    w = lib.Seq2seqDecoderWeights()
    for f in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "attn_out_w", "gen_w", "gen_b"):
        setattr(w, f, 16)
    w.H, w.attn_type, w.VT = 8, lib.S2S_ATTN["dot"], 10
    cw = lib.AcgCopyWeights()
    cw.copy_w = cw.copy_b = 16
    cw.reuse_copy_attn = 1
    ref, cref = C.byref(w), C.byref(cw)
    for name, state in (("nir_acg_beam_decode", [p, p]), ("nir_acg_beam_gru_decode", [p])):
        fn, size = getattr(L, name), getattr(L, name + "_workspace_bytes")

        def call(B=2, QL=7, CV=5, W=3, bytes_=big, pred=p, maps=p):
            return fn(*state, p, p, B, QL, p, 20, 4, None, 2, 6, ref, cref, maps, p, p, CV, W, p, bytes_, pred, p, p, p, None, None)
        for W in (0, 9, 11):
            assert call(W=W) == -1 and b"beam width" in err()
        assert call(CV=1) == -1 and call(CV=1025) == -1 and b"CV outside" in err()
        assert call(bytes_=16) == -3 and b"workspace" in err()
        assert call(pred=None) == -1 and b"null" in err()
        assert call(maps=None) == -1 and b"null" in err()
        assert call(B=0) == 0                                                # nothing enqueued, no device needed
        assert size(2, 7, 5, 3, 6, ref, cref) > 0 and size(2, 7, 5, 9, 6, ref, cref) == 0 and size(2, 7, 1, 3, 6, ref, cref) == 0
        assert size(0, 7, 5, 3, 6, ref, cref) < size(2, 7, 5, 3, 6, ref, cref)
        cw.reuse_copy_attn = 0                                               # a copy attention of its own takes more
        assert size(2, 7, 5, 3, 6, ref, cref) > 0
        cw.reuse_copy_attn = 1
    # the fused form of an empty batch
    w.gen_frag, w.H, w.VT = 16, 32, 100
    assert L.nir_acg_beam_decode(p, p, p, p, 0, 7, p, 20, 4, None, 2, 6, ref, cref, p, p, p, 5, 3, p, big, p, p, p, p, None, None) == 0


# ---- refusals that need no device ---------------------------------------------------------------------------------------------------------------
def test_decode_beam_and_predict_nbest_on_the_cpu():
    import context_attentive_ir_amd.wrappers as Wr
    from context_attentive_ir_amd.config import default_args
    net = AR.case("general")[0]
    with pytest.raises(RuntimeError, match="ROCm device only"):            # no CPU fallback (and no refusal of the copy generator any more)
        net.decode_beam(SRC, LENS, 6, 4, D["src_dict"], D["tgt_dict"], src_map_idx=D["idx"], ext2tgt=D["e2t"], ext2src=D["e2s"])
    net.train()
    with pytest.raises(NotImplementedError, match="eval mode"):
        net.decode_beam(SRC, LENS, 6, 4)
    net.eval()
    kw = dict(src_vocab_size=50, tgt_vocab_size=50, nhid=32, nlayers=1)
    c = Wr.CopyRecommender(default_args("ACG", copy_attn=True, **kw), list(range(50)), list(range(50)))
    with pytest.raises(NotImplementedError, match="predict_nbest"):
        c.predict_beam({}, 4)
    with pytest.raises(AssertionError, match="src_map"):                     # predict_nbest is there and reads the copy fields first
        c.predict_nbest({}, 4)
    s = Wr.SessionRecommender(default_args("HREDQS", bidirection=False, **kw))
    with pytest.raises(NotImplementedError, match="HredQS"):
        s.predict_nbest({}, 4)
    r = Wr.Recommender(default_args("SEQ2SEQ", **kw))
    assert r.predict_nbest.__func__ is Wr.Recommender.predict_nbest and hasattr(r, "predict_beam")
    assert c.network.fuse_generator_topk is True
