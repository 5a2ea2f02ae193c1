"""Host-side (no GPU) checks of teacher-forced scoring under the session models: the teeth of the acceptance criterion (session_score_ref's
planted faults at model level and at the level of the grouped attention), the restatement against a restatement of the suggestion loss at N = 1,
the ranking condition, the registration of the new symbols, their argument checks over fake pointers, and the Python surface."""
import os
import re

import pytest
import torch

import gemm_ref
import score_ref as R
import session_beam_ref as SB
import session_score_ref as SS
from conftest import T, load_golden

N_CAND = 4


@pytest.fixture(scope="module")
def scored():
    """per fixture: (case, candidates, fp64 scores, fp32 chain, the all-fused n_split per token) -- once"""
    out = {}
    for kind, tag in SS.CASES:
        cs = SS.load_case(kind, tag)
        cand = SS.candidates(cs, N_CAND)
        ref = SS.score(cs, cs["sd"], cand)
        chain = SS.score(cs, cs["sd"], cand, dtype=torch.float32)
        out[kind, tag] = (cs, cand, ref, chain, SS.n_split(kind, cand.shape[-1] - 1, True, True))
    return out


# ---- the criterion, model level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", SS.CASES)
def test_the_unfaulted_float32_chain_is_accepted(scored, kind, tag):
    cs, cand, ref, chain, ns = scored[kind, tag]
    ok, fig = SS.accept(chain, ref, chain, 0)
    assert ok, fig
    assert ref["s"] > 1e-3 and int(ref["lengths"].min()) == 1 and int(ref["lengths"].max()) == cand.shape[-1] - 1
    assert len({int(v) for v in ref["lengths"].reshape(-1)}) >= 3              # candidates of unequal lengths
    assert cs["B"] > 1 and cs["SD"] > 1                                        # the pairing quirk can show


@pytest.mark.parametrize("kind,tag", SS.CASES)
def test_the_criterion_rejects_every_fault_at_the_margins_cap(scored, kind, tag):
    cs, cand, ref, chain, ns = scored[kind, tag]
    faults = SS.faults_of(cs)
    assert set(R.FAULTS) - {"no_bias"} <= set(faults) and "state_pairing" in faults
    assert ("wrong_source_row" in faults) == (kind == "cars") and ("sess_dropped" in faults) == (kind == "cars")
    assert ("no_bias" in faults) == (kind != "cars")
    for fault in faults:
        bad = SS.score(cs, cs["sd"], cand, dtype=torch.float32, fault=fault)
        ok, fig = SS.accept(bad, ref, chain, ns, margin=gemm_ref.MARGIN_CAP)
        assert not ok, (kind, tag, fault, fig)


def test_the_margin_may_not_pass_the_cap():
    assert SS.MARGIN <= gemm_ref.MARGIN_CAP
    g = dict(token_logprobs=torch.zeros(1, 1, 2), scores=torch.zeros(1, 1), lengths=torch.zeros(1, 1), s=1.0)
    with pytest.raises(AssertionError):
        SS.accept(g, g, g, 0, margin=2 * gemm_ref.MARGIN_CAP)


# ---- the criterion, attention level -----------------------------------------------------------------------------------------------------------
def _attend_case(seed=5, ngroups=3, G=70, rows_src=5, QL=7, H=32):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(ngroups * G, H, generator=g)
    mem, sb = torch.randn(rows_src, QL, H, generator=g), torch.randn(rows_src, QL, H, generator=g)
    lens = torch.tensor([3, 7, 1, 5, 6])
    rowmap = torch.tensor([4, 0, 2])
    return h, mem, sb, lens, rowmap, G


def test_the_attention_restatement_against_loops():
    h, mem, sb, lens, rowmap, G = _attend_case(G=3)
    ref = SS.tf_attend(h, mem, sb, lens, rowmap, G)
    for r in range(h.shape[0]):
        src = int(rowmap[r // G])
        n = int(lens[src])
        s = [float(h[r].double() @ sb[src, j].double()) for j in range(n)]
        mx = max(s)
        e = [pow(2.718281828459045, v - mx) for v in s]
        a = [v / sum(e) for v in e]
        ctx = sum(a[j] * mem[src, j].double() for j in range(n))
        assert float((ref["cat"][r, :h.shape[1]] - ctx).abs().max()) < 1e-12
        assert ref["attn"][r, n:].tolist() == [0.0] * (mem.shape[1] - n)
        assert torch.equal(ref["cat"][r, h.shape[1]:], h[r].double())
    dead = SS.tf_attend(h, mem, sb, torch.zeros(5, dtype=torch.long), rowmap, G)
    assert bool(torch.isnan(dead["cat"][:, :h.shape[1]]).all()) and bool(torch.isnan(dead["attn"]).all())
    # a map entry outside the bank rows is clamped; a length above QL or below 0 likewise
    far = SS.tf_attend(h, mem, sb, lens, torch.tensor([9, -2, 2]), G)
    near = SS.tf_attend(h, mem, sb, lens, torch.tensor([4, 0, 2]), G)
    assert torch.equal(far["cat"], near["cat"])
    assert torch.equal(SS.tf_attend(h, mem, sb, lens + 100, rowmap, G)["attn"], SS.tf_attend(h, mem, sb, torch.full((5,), 7), rowmap, G)["attn"])


@pytest.mark.parametrize("fault", SS.ATTEND_FAULTS)
def test_the_attention_criterion_rejects_its_faults(fault):
    h, mem, sb, lens, rowmap, G = _attend_case()
    ref = SS.tf_attend(h, mem, sb, lens, rowmap, G)
    chain = SS.tf_attend(h, mem, sb, lens, rowmap, G, torch.float32)
    ok, fig = SS.accept_attend(chain["cat"].float(), chain["attn"].float(), h, ref, chain, 0)
    assert ok, fig
    bad = SS.tf_attend(h, mem, sb, lens, rowmap, G, torch.float32, fault)
    ok, fig = SS.accept_attend(bad["cat"].float(), bad["attn"].float(), h, ref, chain, 2, margin=gemm_ref.MARGIN_CAP)
    assert not ok, (fault, fig)
    if fault == "neighbour_bank":                                               # only the rows of the last block differ
        first = (torch.arange(h.shape[0]) % G) < 64
        assert torch.equal(bad["cat"][first], chain["cat"][first]) and not torch.equal(bad["cat"][~first], chain["cat"][~first])


# ---- the restatement against the loss restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,fixture", SS.TRAIN_CASES)
def test_one_gold_candidate_gives_the_suggestion_loss_restatement(kind, fixture):
    cs = SS.train_case(kind, fixture)
    tseq, twords = cs["target_seq"], cs["target_words"]
    assert cs["B"] > 1 and cs["SD"] > 1
    # behind a gold row's EOS there is PAD alone: the frozen-at-EOS rule changes nothing
    ended = torch.cumsum((tseq[:, 1:] == R.EOS).long(), 1) - (tseq[:, 1:] == R.EOS).long() > 0
    assert bool((tseq[:, 1:][ended] == R.PAD).all())
    out = SS.score(cs, cs["sd"], tseq.unsqueeze(1), rep=twords.unsqueeze(1))
    want = SS.suggestion_nll(cs, cs["sd"], twords, tseq)
    assert float(want) > 0.1
    assert abs(float(-out["scores"].mean()) - float(want)) <= 1e-12 * abs(float(want))
    assert torch.equal(out["lengths"].reshape(-1), (tseq[:, 1:] != R.PAD).sum(1))


# ---- the ranking condition --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", SS.CASES)
def test_the_ranking_fixture_keeps_its_gaps(kind, tag):
    cs = SS.load_case(kind, tag)
    cand = SS.ranking_candidates(cs)
    ref = SS.score(cs, cs["sd"], cand)
    chain = SS.score(cs, cs["sd"], cand, dtype=torch.float32)
    ok, fig = SS.accept(chain, ref, chain, SS.n_split(kind, cand.shape[-1] - 1, True, True))
    bound = SS.score_bound_abs(fig)
    srt = torch.sort(ref["scores"], dim=-1, descending=True)[0]
    gap = float((srt[:, :-1] - srt[:, 1:]).min())
    assert gap >= 10 * bound, (gap, bound)
    ln = ref["lengths"].double()
    srt = torch.sort(ref["scores"] / ln, dim=-1, descending=True)[0]
    assert float((srt[:, :-1] - srt[:, 1:]).min()) >= 10 * bound, "length-normalised"


# ---- symbols and arguments --------------------------------------------------------------------------------------------------------------------
NAMES = {"nir_tf_attend_fusable", "nir_tf_attend_workspace_bytes", "nir_tf_attend"}


def test_new_symbols_exist_with_their_prototypes():
    from conftest import ROOT
    from context_attentive_ir_amd import lib
    main = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    assert '#include "neuroir_teacher.h"' in main
    assert not re.findall(r"\bnir_tf_\w*\s*\(", main)                           # no prototypes of its own, comments included
    hdr = open(os.path.join(ROOT, "include", "neuroir_teacher.h")).read()
    declared = set(re.findall(r"\b(nir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert NAMES == declared == set(lib.TEACHER_SIGNATURES)
    others = (set(lib.SIGNATURES) | set(lib.GRU_DECODE_SIGNATURES) | set(lib.BEAM_SIGNATURES) | set(lib.SESSION_BEAM_SIGNATURES) | set(lib.ACG_BEAM_SIGNATURES)
              | set(lib.HREDQS_BEAM_SIGNATURES) | set(lib.SCORE_SIGNATURES))
    assert not NAMES & others
    L = lib.load()
    for n in NAMES:
        assert hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, hdr, re.S)
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert nargs == len(lib.TEACHER_SIGNATURES[n][1]), n
        assert getattr(L, n).argtypes == lib.TEACHER_SIGNATURES[n][1]           # registered by lib.load


def test_the_fusable_rule():
    from context_attentive_ir_amd import lib
    f = lib.load().nir_tf_attend_fusable
    for same in (0, 1):
        assert f(10, 512, same) == 1 and f(1, 32, same) == 1 and f(64, 64, same) == 1
        assert f(32, 512, same) == 1 and f(33, 512, same) == 0                  # the largest QL at H 512: both banks within 160 KiB of LDS
        assert f(16, 1024, same) == 1 and f(17, 1024, same) == 0
        assert f(65, 32, same) == 0 and f(0, 64, same) == 0
        for H in (36, 16, 48, 1056, 2048, 0, -32):
            assert f(10, H, same) == 0, H


def test_attend_entry_refuses_bad_arguments_before_any_launch():
    """over fake pointers: nothing may be enqueued (no device needed)"""
    from context_attentive_ir_amd import lib
    C = lib.C
    L = lib.load()
    err = lambda: L.nir_last_error_string()                                    # noqa: E731
    p = C.c_void_p(16)

    def att(ngroups=3, G=5, rows_src=4, QL=10, H=64, h=p, mem=p, sb=p, lens=p, rowmap=p, cat=p, attn=None, stride=0, ws=None, nws=0):
        return L.nir_tf_attend(h, mem, sb, lens, rowmap, ngroups, G, rows_src, QL, H, cat, attn, stride, ws, nws, None)
    for kw in (dict(h=None), dict(mem=None), dict(sb=None), dict(lens=None), dict(cat=None)):
        assert att(**kw) == -1 and b"null" in err(), kw
    assert att(ngroups=-1) == -1 and b"negative" in err()
    assert att(G=-1) == -1 and b"negative" in err()
    assert att(ngroups=1 << 20, G=1 << 20) == -1 and b"2^31" in err()
    assert att(rows_src=0) == -1 and b"rows_src" in err()
    assert att(rows_src=-3) == -1 and b"rows_src" in err()
    assert att(rows_src=2, rowmap=None) == -1 and b"rowmap" in err()           # three groups onto two bank rows without a map
    for H in (0, -4, 2, 30, 8196):
        assert att(H=H) == -1 and b"H outside" in err(), H
    for QL in (0, -1, 4097):
        assert att(QL=QL) == -1 and b"QL outside" in err(), QL
    assert att(attn=p, stride=9) == -1 and b"attn_stride" in err()
    assert att(ngroups=0) == 0 and att(G=0) == 0 and att(ngroups=0, rows_src=0) == 0
    assert L.nir_tf_attend_workspace_bytes(160, 180, 10, 512) == 0             # neither form needs scratch today


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------------
def test_score_candidates_and_the_wrapper_on_the_cpu():
    import context_attentive_ir_amd.wrappers as Wr
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.multitask import CARS, M_MATCH_TENSOR, MNSRF
    from helpers import build_model
    for cls in (CARS, M_MATCH_TENSOR, MNSRF):
        assert callable(getattr(cls, "score_candidates"))
    assert callable(getattr(Wr.Multitask, "score_suggestions"))
    for kind, tag in (("cars", "full"), ("mmt", ""), ("mnsrf", "")):
        cs = SS.load_case(kind, tag)
        VT = SS.vocab_tgt(cs)
        net = build_model({"cars": "CARS", "mmt": "M_MATCH_TENSOR", "mnsrf": "MNSRF"}[kind], tgt_vocab_size=VT)
        cand = SS.candidates(cs, 3).view(cs["B"], cs["SD"], 3, -1)
        states = (cs["dec_h"].unsqueeze(0), cs["dec_c"].unsqueeze(0))
        kw = dict(states=states, src_dict=None, tgt_dict=None, batch_size=cs["B"], session_len=cs["SD"])
        if kind == "cars":
            kw.update(encoded_source=cs["enc"], source_len=cs["lens"], session_attns=cs["attns"])
        with pytest.raises(RuntimeError, match="ROCm device only"):            # no CPU fallback
            net.score_candidates(candidate_seq=cand, **kw)
        for bad in (cand[..., :1], cand[:, :1], cand[0], cand.reshape(cs["B"] * cs["SD"], 3, -1)):
            with pytest.raises(ValueError, match="candidate_seq"):
                net.score_candidates(candidate_seq=bad, **kw)
        with pytest.raises(ValueError, match="candidate_rep"):
            net.score_candidates(candidate_seq=cand, candidate_rep=cand[..., :2], **kw)
        net.train()
        with pytest.raises(NotImplementedError, match="eval mode"):
            net.score_candidates(candidate_seq=cand, **kw)
    cs = SS.load_case("cars", "full")
    off = build_model("CARS", tgt_vocab_size=200, turn_recommender_off=True)
    with pytest.raises(RuntimeError, match="turn_recommender_off=False"):      # decode()'s refusal
        off.score_candidates(states=(cs["dec_h"], cs["dec_c"]), candidate_seq=SS.candidates(cs, 2).view(3, 3, 2, -1), src_dict=None, tgt_dict=None, batch_size=3,
                             session_len=3, encoded_source=cs["enc"], source_len=cs["lens"], session_attns=cs["attns"])
    g = load_golden("cars_train")
    V = int(g["meta_vocab"])
    ex = {k: T(g["b0_" + k]) for k in ("source_words", "source_lens", "document_words", "document_lens", "document_labels", "target_words", "target_seq")}
    for model in ("CARS", "M_MATCH_TENSOR", "MNSRF"):
        w = Wr.Multitask(default_args(model, src_vocab_size=V, tgt_vocab_size=V))
        with pytest.raises(RuntimeError, match="ROCm device only"):            # loud without a device, with and without candidates
            w.score_suggestions(ex)
        with pytest.raises(RuntimeError, match="ROCm device only"):
            w.score_suggestions(ex, ex["target_seq"].unsqueeze(2))
