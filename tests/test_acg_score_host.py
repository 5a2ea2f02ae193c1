"""Host-side (no GPU) checks of scoring under ACG's collapsed extended distribution: the float64 restatement (acg_score_ref) against the
fixture computed with the reference's own modules (tests/golden/acg_score.npz), the teeth of the acceptance criterion (eight planted faults),
the registration of the new symbols, their argument checks over fake pointers, extended_targets against the criterion's own gather, and the
Python surface with the refusals that remain."""
import os
import re

import pytest
import torch

import acg_ref as AR
import acg_score_ref as R
import gru_dec_ref as GR
from conftest import T, load_golden

FAULT_CASE = dict(rows=24, rows_per_src=3, K=64, VT=17, CV=9, QL=7, length="mixed")


@pytest.fixture(scope="module")
def batch():
    d = AR.batch_inputs()
    d["e2t"], d["e2s"] = AR.index_tensors(d)
    g = load_golden("acg_score")
    d["cand"], d["rep"], d["lut"] = T(g["candidate_seq"]), T(g["candidate_rep"]), T(g["tgt2src"])
    return d, g


@pytest.fixture(scope="module")
def scored(batch):
    """per fixture case: (state dict, cfg, float64 scores, float32 chain) -- once"""
    d, _ = batch
    out = {}
    for tag in AR.CASES:
        net, cfg, _ = AR.case(tag)
        sd = net.state_dict()
        a = (sd, cfg, d["src"], d["lens"], d["cand"], d["idx"], d["e2t"], d["e2s"])
        out[tag] = (sd, cfg, R.score("lstm", *a, tgt2src=d["lut"]), R.score("lstm", *a, tgt2src=d["lut"], dtype=torch.float32))
    return out


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------------
def test_the_candidates_hold_every_class(batch):
    d, _ = batch
    cand, VT, e2t = d["cand"], len(d["tgt_dict"]), d["e2t"]
    assert torch.equal(cand, R.candidates(d, e2t, VT, cand.shape[2])) and torch.equal(d["rep"], R.default_rep(cand, d["lut"], d["e2s"], VT, len(d["src_dict"])))
    slot = cand >= VT
    c = (cand - VT).clamp(0)
    coll = slot & (e2t.unsqueeze(1).expand(-1, cand.shape[1], -1).gather(2, c.clamp(max=e2t.shape[1] - 1)) >= 0)
    assert bool((slot & ~coll).any())                                          # a copied out-of-vocabulary word
    assert bool(coll.any())                                                    # a collapsed slot id
    in_src = torch.stack([torch.isin(cand[b], d["src"][b, :int(d["lens"][b])]) for b in range(cand.shape[0])])
    assert bool((in_src & (cand >= 4) & ~slot).any()) and bool((~in_src & (cand >= 4) & ~slot).any())       # generated and copied; absent from the source
    assert len({int((row[1:] != AR.PAD).sum()) for row in cand[0]}) >= 3       # unequal lengths


@pytest.mark.parametrize("tag", AR.CASES)
def test_the_restatement_reproduces_the_references_log_probabilities(batch, scored, tag):
    d, g = batch
    sd, cfg, _, _ = scored[tag]
    B, N, TL = d["cand"].shape
    # the fixture records every non-PAD position, those behind an EOS too; the restatement reads 0 there: compared where it counts
    sd64 = {k: v.double() for k, v in sd.items()}
    ref = R.score("lstm", sd64, cfg, d["src"], d["lens"], d["cand"], d["idx"], d["e2t"], d["e2s"], rep=d["rep"])
    rec = T(g["logp_" + tag])
    counted = ref["token_logprobs"] != 0
    assert int(counted.sum()) == int(ref["lengths"].sum()) and float((ref["token_logprobs"] - rec)[counted].abs().max()) <= 1e-6
    assert bool(torch.isfinite(rec).all()) and float(rec.min()) < -3 and float(rec[rec < 0].max()) > -1.5


def test_a_collapsed_slot_id_reads_the_words_value_where_the_reference_holds_1e_10(batch, scored):
    d, g = batch
    rows = T(g["rows_general"])                                                # [B, N, T, VT + CV]
    VT, cand = len(d["tgt_dict"]), d["cand"]
    ref = scored["general"][2]["token_logprobs"]
    seen = 0
    for b in range(cand.shape[0]):
        for n in range(cand.shape[1]):
            ended = False
            for t in range(cand.shape[2] - 1):
                e = int(cand[b, n, t + 1])
                if not ended and e >= VT and e - VT >= 2 and int(d["e2t"][b, e - VT]) >= 0:
                    w = int(d["e2t"][b, e - VT])
                    assert float(rows[b, n, t, e]) == 1e-10                    # the reference's matrix at the slot
                    assert abs(float(ref[b, n, t]) - float(torch.log(rows[b, n, t, w]))) <= 1e-6      # the scorer: the word's value
                    assert abs(float(ref[b, n, t]) - float(torch.log(rows[b, n, t, e]))) > 1.0       # exactly that difference
                    seen += 1
                ended = ended or e == AR.EOS
    assert seen >= cand.shape[0]


@pytest.mark.parametrize("tag", AR.CASES)
def test_the_gold_target_gives_the_references_loss(batch, tag):
    d, g = batch
    net, cfg, _ = AR.case(tag)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    VT = len(d["tgt_dict"])
    gold_p = T(g["gold_p_" + tag])
    counted = d["ts"][:, 1:] != AR.PAD
    assert float(gold_p[counted].min()) > 1e-12                                # the criterion's 1e-20 cannot matter
    cand = R.extended_targets(d["ts"], d["al"], VT).unsqueeze(1)
    out = R.score("lstm", sd, cfg, d["src"], d["lens"], cand, d["idx"], d["e2t"], d["e2s"], rep=d["tw"].unsqueeze(1))
    # the loss masks PAD only; the scorer also freezes behind EOS -- the fixture's gold rows hold no EOS, so both count the same tokens
    assert torch.equal(out["lengths"].squeeze(1), counted.sum(1))
    loss = float(-out["scores"].mean())
    assert abs(loss - float(g["loss_" + tag])) <= 1e-6 * abs(float(g["loss_" + tag]))
    assert abs(float(g["loss_" + tag]) - float(load_golden("acg")["loss_" + tag])) <= 1e-4 * abs(loss)      # the fp32 record of the same loss
    assert float((torch.exp(out["token_logprobs"].squeeze(1)) - gold_p)[counted].abs().max()) <= 1e-9


# ---- the criterion ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", AR.CASES)
def test_the_unfaulted_float32_chain_is_accepted(scored, tag):
    _, _, ref, chain = scored[tag]
    ok, fig = R.accept(chain, ref, chain, 0)
    assert ok, fig
    assert ref["s"] > 1e-3 and len({int(v) for v in ref["lengths"].reshape(-1)}) >= 3


@pytest.mark.parametrize("fault", R.GEN_FAULTS)
def test_the_generator_level_criterion_rejects_its_faults(fault):
    c = R.planted(**FAULT_CASE)
    ref, chain = R.planted_ref(c), R.planted_ref(c, torch.float32)
    s = float(ref[1].abs().max())
    ok, fig = R.accept_rows(chain[0], ref[0], chain[0], s, 0)
    assert ok and int(torch.isneginf(ref[0]).sum()) == c["n_inf"] > 0, fig
    bad = R.planted_ref(c, torch.float32, fault)
    ok, fig = R.accept_rows(bad[0], ref[0], chain[0], s, 2, margin=R.MARGIN_CAP)
    assert not ok, (fault, fig)


@pytest.mark.parametrize("fault", ["shift", "no_pad_sub", "no_collapse_mass", "swap_switch", "wrong_src_row", "slot_not_canonical"])
def test_the_model_level_criterion_rejects_the_faults_a_fixture_shows(batch, scored, fault):
    d, _ = batch
    sd, cfg, ref, chain = scored["general"]
    bad = R.score("lstm", sd, cfg, d["src"], d["lens"], d["cand"], d["idx"], d["e2t"], d["e2s"], tgt2src=d["lut"], dtype=torch.float32, fault=fault)
    ns = R.n_path(d["src"].shape[1], d["cand"].shape[2] - 1) + 2
    ok, fig = R.accept(bad, ref, chain, ns, margin=R.MARGIN_CAP)
    assert not ok, (fault, fig)


def test_the_fault_list_and_the_margin():
    assert len(R.FAULTS) == 8 and set(R.GEN_FAULTS) | {"shift"} == set(R.FAULTS)
    assert R.MARGIN <= R.MARGIN_CAP == 4.0
    c = R.planted(**FAULT_CASE)
    with pytest.raises(AssertionError):
        R.accept_rows(R.planted_ref(c)[0], R.planted_ref(c)[0], R.planted_ref(c)[0], 1.0, 0, margin=8.0)
    assert {R.CLASSES[i] for i in c["classes"].tolist()} == set(R.CLASSES)      # the fault case holds every target class


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_the_restatement_of_the_rows_is_acg_refs(dtype):
    c = R.planted(**FAULT_CASE)
    rows = torch.arange(c["o"].shape[0]) // c["rows_per_src"]
    sd = R._sd(c["gen_w"], c["gen_b"], c["copy_w"], c["copy_b"], dtype)
    a = (sd, c["o"].to(dtype), c["attn"].to(dtype), c["smap"][rows], c["lens"][rows], c["e2t"].shape[1])
    VT = c["gen_w"].shape[0]
    (P, l), (Pw, lw) = R.extended_rows(*a), AR.extended(*a)
    assert torch.equal(l, lw) and torch.equal(P[:, VT:], Pw[:, VT:])            # the logits and the copy part: the same operations in the same order
    assert float(((P - Pw)[:, :VT] / Pw[:, :VT]).abs().max()) <= 4 * torch.finfo(dtype).eps      # sigmoid(-x) against 1 - sigmoid(x) at x ~ 0


def test_a_minus_infinity_elsewhere_is_rejected():
    c = R.planted(**FAULT_CASE)
    ref, chain = R.planted_ref(c), R.planted_ref(c, torch.float32)
    got = chain[0].clone()
    got[int((c["classes"] == R.CLASSES.index("word_no_mass")).nonzero()[0])] = float("-inf")
    assert not R.accept_rows(got, ref[0], chain[0], float(ref[1].abs().max()), 2, margin=R.MARGIN_CAP)[0]


# ---- extended_targets ----------------------------------------------------------------------------------------------------------------------------------
def test_extended_targets_is_where_the_criterion_finds_a_gold_token(batch):
    """a direct gather of a reference-style [.., VT + CV] matrix (not collapsed) at the criterion's two places against ONE read of the collapsed
    matrix at extended_targets: equal up to the criterion's 1e-20"""
    from context_attentive_ir_amd.recommender.acg import extended_targets
    d, _ = batch
    VT, CV = len(d["tgt_dict"]), d["e2t"].shape[1]
    ts, al = d["ts"][:, 1:], d["al"][:, 1:]
    ext = extended_targets(d["ts"], d["al"], VT)
    assert torch.equal(ext, R.extended_targets(d["ts"], d["al"], VT)) and bool((ext >= VT).any()) and bool(((ext < VT) & (d["al"] > 1)).any())
    assert torch.equal(extended_targets(d["ts"], d["al"][:, :-2], VT)[:, :-2], ext[:, :-2])                  # a short alignment is padded with 0
    g = torch.Generator().manual_seed(5)
    B, TL1 = ts.shape
    P = torch.rand(B, TL1, VT + CV, generator=g, dtype=torch.float64)
    for b in range(B):                                                          # mass only at slots the row's source holds, as copy_generator leaves it
        held = set(d["idx"][b, :int(d["lens"][b])].tolist())
        P[b, :, [VT + c for c in range(CV) if c not in held]] = 0
    anu, au = (al != AR.UNK).double(), (al == AR.UNK).double()
    out = P.gather(2, (al + VT).unsqueeze(2)).squeeze(2) * anu + AR.EPS_LOSS + P.gather(2, ts.unsqueeze(2)).squeeze(2) * (
        (ts != AR.UNK).double() + au * (ts == AR.UNK).double())
    C = P.clone()
    for t in range(TL1):
        C[:, t] = AR.collapse_(C[:, t].clone(), d["e2t"], VT)
    e = ext[:, 1:]
    canon = R.canonical(e.reshape(-1), d["e2t"].repeat_interleave(TL1, 0), VT).view(B, TL1)
    mine = C.gather(2, canon.unsqueeze(2)).squeeze(2)
    counted = ts != AR.PAD
    assert float((mine - out)[counted].abs().max()) <= 2 * AR.EPS_LOSS + 1e-15


# ---- symbols and arguments ----------------------------------------------------------------------------------------------------------------------------
NAMES = {"nir_acg_score_gen_target_workspace_bytes", "nir_acg_score_gen_target"}


def test_new_symbols_exist_with_their_prototypes():
    from conftest import ROOT
    from context_attentive_ir_amd import lib
    main = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    assert '#include "neuroir_acg_score.h"' in main
    assert not re.findall(r"\bnir_acg_score\w*\s*\(", main)                     # no prototypes of its own, comments included
    hdr = open(os.path.join(ROOT, "include", "neuroir_acg_score.h")).read()
    declared = set(re.findall(r"\b(nir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert NAMES == declared == set(lib.ACG_SCORE_SIGNATURES)
    others = (set(lib.SIGNATURES) | set(lib.GRU_DECODE_SIGNATURES) | set(lib.BEAM_SIGNATURES) | set(lib.SESSION_BEAM_SIGNATURES) | set(lib.ACG_BEAM_SIGNATURES)
              | set(lib.HREDQS_BEAM_SIGNATURES) | set(lib.SCORE_SIGNATURES) | set(lib.TEACHER_SIGNATURES) | set(lib.SAMPLE_SIGNATURES)
              | set(lib.SESSION_SAMPLE_SIGNATURES))
    assert not NAMES & others
    L = lib.load()
    for n in NAMES:
        assert hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, hdr, re.S)
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert nargs == len(lib.ACG_SCORE_SIGNATURES[n][1]), n
        assert getattr(L, n).argtypes == lib.ACG_SCORE_SIGNATURES[n][1]         # registered by lib.load


def test_the_entry_refuses_bad_arguments_before_any_launch():
    """over fake pointers: nothing may be enqueued (no device needed)"""
    from context_attentive_ir_amd import lib
    C = lib.C
    L = lib.load()
    err = lambda: L.nir_last_error_string()                                    # noqa: E731
    p, big = C.c_void_p(16), 1 << 40
    size = L.nir_acg_score_gen_target_workspace_bytes

    def gen(rows=6, rps=3, K=64, VT=40, QL=7, CV=9, stride=7, ws=big, o=p, w=p, frag=p, cw=p, cb=p, at=p, ln=p, mp=p, et=p, tg=p, out=p, wsp=p):
        return L.nir_acg_score_gen_target(o, rows, rps, K, w, p, frag, VT, cw, cb, at, stride, ln, QL, mp, et, CV, tg, 0, wsp, ws, out, None, None)
    for kw in (dict(o=None), dict(w=None), dict(cw=None), dict(cb=None), dict(at=None), dict(ln=None), dict(mp=None), dict(et=None), dict(tg=None),
               dict(out=None)):
        assert gen(**kw) == -1 and b"null" in err(), kw
    assert gen(rows=-1) == -1 and b"rows" in err()
    assert gen(rows=1 << 31, rps=1) == -1 and b"rows" in err()
    for rps in (0, -1, 4, 12):                                                  # at least 1, and a divisor of rows
        assert gen(rps=rps) == -1 and b"rows_per_src" in err(), rps
    for K in (0, -4, 2, 30, 8196):
        assert gen(K=K) == -1 and b"K outside" in err(), K
        assert size(6, K, 40, 0) == 0 and size(6, K, 40, 1) == 0
    for VT in (0, -1, (1 << 31) - 16 - 1024):
        assert gen(VT=VT) == -1 and b"VT" in err(), VT
        assert size(6, 64, VT, 1) == 0
    for kw in (dict(QL=0), dict(QL=4097, stride=4097), dict(CV=1), dict(CV=1025)):
        assert gen(**kw) == -1 and b"QL outside" in err(), kw
    assert gen(stride=6) == -1 and b"attn_stride" in err()
    for frag in (p, None):                                                      # both forms: a short or a null workspace
        assert gen(ws=16, frag=frag) == -3 and b"workspace" in err()
        assert gen(wsp=None, frag=frag) == -3 and b"workspace" in err()
        assert gen(rows=0, frag=frag) == 0 and gen(rows=0, frag=frag, wsp=None, ws=0) == 0
    assert size(0, 64, 40, 1) == 0
    score = L.nir_score_gen_target_workspace_bytes                               # the form's own buffers + two int32 ids a row (+ one partial, plain)
    assert size(24320, 512, 30000, 1) == score(24320, 512, 30000, 1) + 2 * 24320 * 4 < 64 << 20
    assert size(100, 512, 30000, 0) == score(100, 512, 30000, 0) + 2 * 512 + 2 * 512
    assert size(5, 48, 40, 1) == size(5, 48, 40, 0) > 0                         # a K without a fragment form: the plain form's size
    assert size((1 << 18) + 5, 64, 40, 1) - size(1 << 18, 64, 40, 1) == 2 * 256  # rows beyond a chunk reuse the chunk's partials: only the ids grow


# ---- the Python surface -------------------------------------------------------------------------------------------------------------------------------
def test_score_extended_and_the_refusals_that_remain_on_the_cpu(batch):
    import context_attentive_ir_amd.wrappers as Wr
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.recommender import ACG, ACGGRU
    d, _ = batch
    maps = dict(src_map_idx=d["idx"], ext2tgt=d["e2t"], ext2src=d["e2s"])
    for cls in (ACG, ACGGRU):
        assert callable(getattr(cls, "score_extended"))
    assert callable(Wr.CopyRecommender.score_extended)
    nets = (AR.case("general")[0], GR.case("acg", "general")[0])
    for net in nets:
        with pytest.raises(NotImplementedError, match="extended distribution"):     # target-vocabulary ids: still another model's number
            net.score_candidates(d["src"], d["lens"], d["cand"])
        with pytest.raises(NotImplementedError, match="score_extended"):
            net.score_candidates(d["src"], d["lens"], d["cand"])
        with pytest.raises(RuntimeError, match="ROCm device only"):                  # no CPU fallback
            net.score_extended(d["src"], d["lens"], d["cand"], **maps)
        with pytest.raises(ValueError, match="candidate_seq"):
            net.score_extended(d["src"], d["lens"], d["cand"][:, :, :1], **maps)
        with pytest.raises(ValueError, match="candidate_seq"):
            net.score_extended(d["src"], d["lens"], d["cand"][:2], **maps)
        with pytest.raises(ValueError, match="candidate_rep"):
            net.score_extended(d["src"], d["lens"], d["cand"], candidate_rep=d["cand"][:, :1], **maps)
        net.train()
        with pytest.raises(NotImplementedError, match="eval mode"):
            net.score_extended(d["src"], d["lens"], d["cand"], **maps)
        net.eval()
    kw = dict(src_vocab_size=50, tgt_vocab_size=50, nhid=32)
    c = Wr.CopyRecommender(default_args("ACG", nlayers=1, **kw))
    with pytest.raises(NotImplementedError, match="extended distribution"):
        c.score({})
    with pytest.raises(NotImplementedError, match="score_extended"):
        c.score({})
    with pytest.raises(AssertionError, match="src_map"):
        c.score_extended({"source_words": d["src"]})
